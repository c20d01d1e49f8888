"""CPU-only checks of the two-sample statistics: the pure-numpy definitions of utils/twosample.py (the unbiased MMD^2 against
a double loop, the label generators, the p-value formula with ties), the yardstick of the GPU tests on its own
(twosamplecommon: integer data gives integers, the bound is positive where a form has terms), the ctypes table against
include/siggan_twosample.h, the workspace size and every refusal of siggan_kernel_forms (argument checks in front of any HIP
call, so they run without a GPU), the Python layer's refusals, and the CLI's new flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import twosamplecommon as TC
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils import twosample as TS


def test_mmd2_from_forms_against_a_double_loop():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((7, 3)), rng.standard_normal((5, 3))
    k = lambda u, v: (u @ v / 3 + 1.0) ** 3                              # noqa: E731
    faa = sum(k(a[i], a[j]) for i in range(7) for j in range(7) if i != j)
    fbb = sum(k(b[i], b[j]) for i in range(5) for j in range(5) if i != j)
    fab = sum(k(a[i], b[j]) for i in range(7) for j in range(5))
    want = faa / (7 * 6) + fbb / (5 * 4) - 2 * fab / (7 * 5)
    got = TS.mmd2_from_forms([[faa, fbb, fab], [0.0, 0.0, 0.0]], 7, 5)
    assert got.shape == (2,) and got[0] == pytest.approx(want, rel=1e-14) and got[1] == 0.0
    # the same through the yardstick's forms of the pooled rows
    x = np.concatenate([a, b]).astype(np.float32)
    labels = np.array([1] * 7 + [2] * 5, np.uint8)[:, None]
    f, bound, _ = TC.forms(x, labels, "poly", 1.0 / 3, 1.0, 3)
    value, vb = TC.mmd2(f, bound, 7, 5)
    assert TS.mmd2_from_forms(f, 7, 5)[0] == pytest.approx(value[0], abs=vb[0]) and 0 < vb[0] < 1e-12
    for na, nb in ((1, 5), (7, 1), (0, 0)):
        with pytest.raises(ValueError, match="at least 2"):
            TS.mmd2_from_forms(f, na, nb)


def test_permutation_labels():
    lab = TS.permutation_labels(7, 5, 30, seed=3)
    assert lab.dtype == np.uint8 and lab.shape == (12, 31)
    assert lab[:, 0].tolist() == [1] * 7 + [2] * 5
    assert ((lab == 1).sum(axis=0) == 7).all() and ((lab == 2).sum(axis=0) == 5).all()
    assert len({c.tobytes() for c in lab.T}) > 25                         # they ARE permuted
    assert np.array_equal(lab, TS.permutation_labels(7, 5, 30, seed=3))
    assert not np.array_equal(lab, TS.permutation_labels(7, 5, 30, seed=4))
    assert np.array_equal(lab[:, :11], TS.permutation_labels(7, 5, 10, seed=3))     # more permutations extend the same sequence


def test_subset_labels():
    lab = TS.subset_labels(9, 6, 40, 4, seed=1)
    assert lab.dtype == np.uint8 and lab.shape == (15, 40) and set(np.unique(lab)) == {0, 1, 2}
    assert ((lab[:9] == 1).sum(axis=0) == 4).all() and ((lab[9:] == 2).sum(axis=0) == 4).all()
    assert not (lab[:9] == 2).any() and not (lab[9:] == 1).any()            # no row carries two labels or the other set's
    assert np.array_equal(lab, TS.subset_labels(9, 6, 40, 4, seed=1)) and not np.array_equal(lab, TS.subset_labels(9, 6, 40, 4, seed=2))
    full = TS.subset_labels(9, 6, 3, 6, seed=1)
    assert (full[9:] == 2).all()                                           # subset_size = n_fake takes every generated row
    for kw in (dict(subset_size=1), dict(subset_size=7), dict(subsets=0)):
        with pytest.raises(ValueError):
            TS.subset_labels(9, 6, **{**dict(subsets=3, subset_size=4, seed=0), **kw})


def test_p_value_counts_ties():
    assert TS.p_value([0.5, 0.1, 0.2, 0.3]) == 1 / 4
    assert TS.p_value([0.5, 0.5, 0.2, 0.9]) == 3 / 4                       # >= : the tie counts
    assert TS.p_value([0.5, 0.6, 0.7, 0.5, 0.5]) == 1.0
    assert TS.p_value([-1.0, -2.0]) == 1 / 2
    with pytest.raises(ValueError):
        TS.p_value([0.5])


def test_median_heuristic():
    rows = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 8.0]], np.float32)      # d2: 25, 100, 25
    assert TS.median_heuristic_gamma(rows) == 1 / 25 == TC.median_gamma(rows)
    with pytest.raises(ValueError, match="median"):
        TS.median_heuristic_gamma(np.zeros((4, 3), np.float32))


def test_yardstick_on_integer_data_gives_integers():
    x, labels = TC.integer_rows(131, 40), TC.random_labels(131, 17)
    k, _ = TC.kernel_matrix(x, "poly", 1.0, 0.0, 3)
    print(f"largest |k| at n = 131, dim = 40: {np.abs(k).max():.3e}")
    f, bound, diag = TC.forms(x, labels, "poly", 1.0, 0.0, 3)
    assert np.array_equal(f, np.round(f)) and np.abs(f).max() < 2.0 ** 53 and np.array_equal(diag, ((x.astype(np.float64) ** 2).sum(1)) ** 3)
    a, b = labels == 1, labels == 2
    p = 5
    direct = [sum(k[i, j] for i in np.flatnonzero(s[:, p]) for j in np.flatnonzero(t[:, p]) if i != j) for s, t in ((a, a), (b, b), (a, b))]
    assert f[p].tolist() == direct
    assert (bound > 0).all()


def test_python_layer_refusals():
    for n_real, n_fake in ((1, 5), (5, 1), (0, 0)):
        with pytest.raises(ValueError, match="at least 2"):
            TS.permutation_labels(n_real, n_fake, 10, 0)
    with pytest.raises(ValueError, match="SIGGAN_TWOSAMPLE_MAX_N"):
        TS.permutation_labels(_lib.TWOSAMPLE_MAX_N, 2, 1, 0)
    with pytest.raises(ValueError, match="SIGGAN_TWOSAMPLE_MAX_N"):
        TS.subset_labels(2, _lib.TWOSAMPLE_MAX_N - 1, 1, 2, 0)
    with pytest.raises(ValueError):
        TS.permutation_labels(5, 5, 0, 0)
    with pytest.raises(ValueError, match="kind"):
        TS.kernel_spec("linear", 1.0)


def test_wrappers_refuse_without_a_device():
    x, lab = torch.zeros(9, 8), torch.zeros(9, 2, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU path"):
        TS.kernel_forms(x, lab, kind="poly", gamma=1.0)
    with pytest.raises(ValueError, match="no CPU path"):
        TS.kid(x, x)
    with pytest.raises(ValueError, match="no CPU path"):
        TS.mmd_permutation_test(x, x)
    from signature_gan_amd.utils.metrics import two_sample_metrics
    with pytest.raises(ValueError, match="no CPU path"):
        two_sample_metrics(x, x)


def test_library_exports_the_twosample_header():
    with open(os.path.join(ROOT, "include", "siggan_twosample.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(?:int|size_t)\s+(siggan_\w+)\s*\(", header))
    assert declared == set(_lib.TWOSAMPLE_EXPORTS) == {"siggan_kernel_forms", "siggan_kernel_forms_workspace"}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in siggan_twosample.h but not exported"
    assert lib.siggan_abi_version() == 4                                   # symbols only added
    assert not set(_lib.TWOSAMPLE_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 64
    for name, value in (("MAX_N", _lib.TWOSAMPLE_MAX_N), ("MAX_COLS", _lib.TWOSAMPLE_MAX_COLS), ("MAX_DIM", _lib.TWOSAMPLE_MAX_DIM),
                        ("ROW_BLOCK", _lib.TWOSAMPLE_ROW_BLOCK)):
        assert int(re.search(rf"#define SIGGAN_TWOSAMPLE_{name}\s+(\d+)", header).group(1)) == value
    assert re.search(r"SIGGAN_KERNEL_POLY = 0, SIGGAN_KERNEL_RBF = 1", header) and (_lib.KERNEL_POLY, _lib.KERNEL_RBF) == (0, 1)
    assert C.sizeof(_lib.KernelSpec) == 24 and _lib.KernelSpec.gamma.offset == 8 and _lib.KernelSpec.coef0.offset == 16


def test_workspace_size():
    lib = _lib.load()
    ws = lib.siggan_kernel_forms_workspace
    assert ws(0, 1) == ws(1, 0) == ws(-1, 1) == ws(_lib.TWOSAMPLE_MAX_N + 1, 1) == ws(1, _lib.TWOSAMPLE_MAX_COLS + 1) == 0
    assert ws(1, 1) == 24 + 8 and ws(32, 1) == 24 + 256 and ws(33, 1) == 48 + 264 and ws(33, 7) == 48 * 7 + 264    # partials, then n norms
    assert ws(4096, 1024) == 24 * 128 * 1024 + 8 * 4096 == 3 * 2 ** 20 + 2 ** 15     # "a few MB" at the evaluation's large shape


def test_every_refusal_comes_before_any_device_call():
    """Host memory stands in for every pointer: a refused call dereferences none and launches nothing."""
    lib = _lib.load()
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    size = lib.siggan_kernel_forms_workspace(9, 5)

    def call(x=ptr, n=9, dim=8, kind=0, degree=3, gamma=1.0, coef0=1.0, labels=ptr, cols=5, forms=ptr, diag=ptr, ws=ptr, ws_bytes=size,
             spec=True):
        s = _lib.KernelSpec(kind, degree, gamma, coef0)
        return lib.siggan_kernel_forms(0, x, n, dim, C.byref(s) if spec else None, labels, cols, forms, diag, ws, ws_bytes, None)

    bad = [(dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=_lib.TWOSAMPLE_MAX_N + 1, ws_bytes=1 << 40), b"n ="),
           (dict(cols=0), b"cols"), (dict(cols=_lib.TWOSAMPLE_MAX_COLS + 1, ws_bytes=1 << 40), b"cols"), (dict(dim=0), b"dim"),
           (dict(dim=_lib.TWOSAMPLE_MAX_DIM + 1), b"dim"), (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"), (dict(degree=0), b"degree"),
           (dict(degree=4), b"degree"), (dict(gamma=0.0), b"gamma"), (dict(gamma=-0.5), b"gamma"), (dict(gamma=float("nan")), b"gamma"),
           (dict(gamma=float("inf")), b"gamma"), (dict(coef0=float("nan")), b"coef0"), (dict(coef0=float("inf")), b"coef0"),
           (dict(x=None), b"null"), (dict(labels=None), b"null"), (dict(forms=None), b"null"), (dict(spec=False), b"null"),
           (dict(ws=None), b"workspace"), (dict(ws_bytes=size - 1), b"workspace"), (dict(ws_bytes=0), b"workspace"),
           (dict(ws=C.c_void_p(ptr.value + 4)), b"aligned")]
    for kw, word in bad:
        assert call(**kw) == _lib.E_ARG, kw
        assert word in lib.siggan_last_error(), (kw, lib.siggan_last_error())
        with pytest.raises(ValueError, match="siggan_kernel_forms"):
            _lib.check(_lib.E_ARG)


def test_cli_flag_parses_and_stays_out_of_the_way():
    from signature_gan_amd.evaluate_vanilla_gan_signatures import parse_args
    plain = parse_args(["--checkpoint", "ck.pt"])
    assert "verifier_kid" not in vars(plain) and plain.verifier_kid is None
    assert parse_args(["--checkpoint", "ck.pt", "--verifier_kid"]).verifier_kid == 1000
    assert parse_args(["--checkpoint", "ck.pt", "--verifier_kid", "99"]).verifier_kid == 99
    with pytest.raises(SystemExit):
        parse_args(["--checkpoint", "ck.pt", "--verifier_kid", "0"])
