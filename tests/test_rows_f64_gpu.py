"""What csrc/rows_f64.h exists for, on the MI355X: neighbors.hip and twosample.hip sum a row's products in ONE chunk and step
order, so they agree with each other -- not only each with numpy (test_neighbors_gpu.py, test_twosample_gpu.py).

Everything here is exact: a row against a bit-identical row gives d2 = 0.0 in knn and k = 1.0 under the RBF kernel, whatever
tile either row sits in; |x|^2 out of knn (the distance to a zero row) and out of kernel_forms (the degree-1 kernel's
diagonal) are the same bits; and the 16-byte loader and the scalar one give the same bits in both ops.

Shapes: n = 15, 16, 17, 33 (a ragged tile, a full one, a second tile of one row, a third tile: with four waves per workgroup
in k_forms and one tile per wave in k_neighbors, 33 rows reach a second and third wave); dim = 1, 3 (inside one MFMA step),
4 (one step, 16-byte loads allowed), 17 (a chunk and a ragged second one), 20 (the same with 16-byte loads).  Every set once
16-byte aligned and once 4 bytes past it, where only the scalar loader is allowed."""
import functools

import numpy as np
import pytest
import torch

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd.utils.neighbors import knn
from signature_gan_amd.utils.twosample import kernel_forms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, DIMS = (15, 16, 17, 33), (1, 3, 4, 17, 20)
GAMMA = 0.5


def place(rows: np.ndarray, offset: bool) -> torch.Tensor:
    """The rows on the device, 16-byte aligned or 4 bytes past that."""
    n, dim = rows.shape
    flat = torch.empty(n * dim + 1, dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    t = flat[1:] if offset else flat[:-1]
    t = t.view(n, dim)
    t.copy_(torch.from_numpy(rows))
    assert t.is_contiguous() and t.data_ptr() % 16 == (4 if offset else 0)
    return t


def bits(t: torch.Tensor) -> bytes:
    return t.cpu().contiguous().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def run(n: int, dim: int, offset: bool):
    """Every result of one set, computed once: rows n - 1 and 0 are the same row (another tile for n > 16)."""
    rng = np.random.default_rng([n, dim])
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    plain = place(rows, offset)
    rows[n - 1] = rows[0]
    dup = place(rows, offset)
    labels = rng.integers(0, 3, size=(n, 3)).astype(np.uint8)
    labels[:, 0] = 0
    labels[0, 0], labels[n - 1, 0] = 1, 2                                # column 0: the pair (row 0, its copy) alone
    labels = torch.from_numpy(labels).to(DEV)
    zero = torch.zeros(1, dim, dtype=torch.float32, device=DEV)
    out = {"self": knn(plain, plain, 1), "dup": knn(dup, dup, 1, exclude_self=True), "norm": knn(dup, zero, 1),
           "rbf": kernel_forms(dup, labels, kind="rbf", gamma=GAMMA, want_diag=True),
           "linear": kernel_forms(dup, labels, kind="poly", gamma=1.0, coef0=0.0, degree=1, want_diag=True)}
    torch.cuda.synchronize()
    return {k: tuple(t.cpu() for t in v) for k, v in out.items()}


CASES = [(n, dim) for n in NS for dim in DIMS]
ids = lambda c: f"n{c[0]}_dim{c[1]}"                                      # noqa: E731


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_a_row_is_at_distance_zero_from_itself_and_from_its_copy_in_both_ops(case, offset):
    n, dim = case
    r = run(n, dim, offset)
    d2, index = r["self"]
    assert bits(d2) == bits(torch.zeros(n, 1, dtype=torch.float64)), d2.reshape(-1).tolist()       # exactly +0.0
    assert index.reshape(-1).tolist() == list(range(n))
    d2, index = r["dup"]
    assert d2[0, 0].item() == 0.0 and index[0, 0].item() == n - 1 and d2[n - 1, 0].item() == 0.0 and index[n - 1, 0].item() == 0
    assert (d2[1:n - 1] > 0).all()                                        # and nobody else is anybody's copy
    forms, diag = r["rbf"]
    assert bits(diag) == bits(torch.ones(n, dtype=torch.float64)), diag.tolist()                   # exactly 1.0
    assert forms[0].tolist() == [0.0, 0.0, 1.0]                           # k(row 0, its copy) across tiles: exactly 1.0


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_two_ops_give_the_same_bits_for_a_rows_squared_norm(case, offset):
    """knn's |q|^2 (the distance to a zero row: (|q|^2 + 0) - 2 * 0) against kernel_forms' x_i . x_i (degree 1, gamma 1,
    coef0 0): two kernels in two files, one order of summation."""
    r = run(*case, offset)
    d2, _ = r["norm"]
    forms, diag = r["linear"]
    assert bits(d2.reshape(-1)) == bits(diag), (d2.reshape(-1) - diag).abs().max().item()
    assert forms[0, 2].item() == diag[0].item()                           # row 0 . its copy, off the diagonal tile for n > 16


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_aligned_and_offset_rows_give_equal_bits_in_both_ops(case):
    a, b = run(*case, False), run(*case, True)
    assert a.keys() == b.keys()
    for name in a:
        for ta, tb in zip(a[name], b[name]):
            assert ta.dtype == tb.dtype and bits(ta) == bits(tb), name
