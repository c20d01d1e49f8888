"""Two-sample statistics between two sets of feature vectors that stay on the device: the Kernel Inception Distance and a
permutation test of the kernel MMD.

A Frechet distance over 128-dimensional embeddings (utils/frechet.py) estimates a 128 x 128 covariance from a few hundred
rows; it is biased upwards by an amount that depends on N, so two evaluations with different ``--n_samples`` cannot be
compared, and it carries no error bar.  The figures here do not have that fault:

* ``kid``: the unbiased MMD^2 estimator under the cubic polynomial kernel (Binkowski et al. 2018), reported as mean and
  standard deviation over random subsets, plus the estimator on the full sets.  Unbiased at any N.
* ``mmd_permutation_test``: the same estimator (RBF kernel by default, bandwidth by the median heuristic) on the observed
  labelling and on label permutations of the pooled rows: a p-value for "the two sets come from one distribution" that means
  the same at N = 200 as at N = 20 000.

Both are made of one primitive, ``kernel_forms`` (include/siggan_twosample.h, csrc/twosample.hip): for every column of a
label matrix -- 0 neither, 1 group A, 2 group B -- the sums of k(x_i, x_j) over the ordered pairs inside A, inside B and
between them, the diagonal left out by row number, in fp64 on the device without forming the (n, n) kernel matrix.  A subset
is a column, a permutation is a column; three numbers per column reach the host, where ``mmd2_from_forms`` -- pure numpy, the
definition in one place -- turns them into the statistic.

A caveat on KID here: the verifier's embeddings are unit-norm at dim 128, so with the literature's gamma = 1 / dim the
argument gamma * a.b + 1 stays within 1 +- 1/128 and the cubic kernel is almost linear: KID then mostly compares the two
sets' MEANS.  The RBF permutation test is the sharper instrument, and ``gamma`` is there to be raised."""
import ctypes as C
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch

from .. import _lib
from .._call import check_rows, ptr, stream

KINDS = {"poly": _lib.KERNEL_POLY, "rbf": _lib.KERNEL_RBF}
MEDIAN_ROWS = 512                                          # the median heuristic looks at no more pooled rows than this
KID_MAX_SUBSET = 1000


# ---- the device call ---------------------------------------------------------------------------------------------------
def _check_inputs(x: torch.Tensor, labels: torch.Tensor) -> torch.device:
    check_rows("x", x, torch.float32, "(n, dim)")
    check_rows("labels", labels, torch.uint8, f"({x.shape[0]}, cols)", shape=(x.shape[0], None), device=x.device,
               where=f"x's device {x.device}")
    if x.shape[0] > _lib.TWOSAMPLE_MAX_N:
        raise ValueError(f"n = {x.shape[0]} rows exceed SIGGAN_TWOSAMPLE_MAX_N = {_lib.TWOSAMPLE_MAX_N}")
    return x.device


def kernel_spec(kind: str, gamma: float, coef0: float = 1.0, degree: int = 3) -> "_lib.KernelSpec":
    if kind not in KINDS:
        raise ValueError(f"kind must be 'rbf' or 'poly', got {kind!r}")
    return _lib.KernelSpec(KINDS[kind], int(degree), float(gamma), float(coef0))


def kernel_forms(x: torch.Tensor, labels: torch.Tensor, kind: str = "rbf", gamma: float = 1.0, coef0: float = 1.0, degree: int = 3,
                 want_diag: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """fp64 (cols, 3): for every column p of ``labels`` (uint8 (n, cols): 1 = group A, 2 = group B, anything else neither)
    the sums of k(x_i, x_j) over the ordered pairs i != j inside A_p, inside B_p, and over i in A_p, j in B_p, for the rows
    of ``x`` (n, dim) fp32.  'poly': k = (gamma a.b + coef0)^degree, degree 1 .. 3; 'rbf': k = exp(-gamma |a - b|^2).
    ``want_diag``: -> (forms, diag) with diag fp64 (n) = k(x_i, x_i).  Both tensors contiguous on one ROCm device; columns
    beyond SIGGAN_TWOSAMPLE_MAX_COLS go in several calls; nothing synchronises the host."""
    dev = _check_inputs(x, labels)
    spec = kernel_spec(kind, gamma, coef0, degree)
    lib = _lib.load()
    n, dim, cols = x.shape[0], x.shape[1], labels.shape[1]
    forms = torch.empty(cols, 3, dtype=torch.float64, device=dev)
    diag = torch.empty(n, dtype=torch.float64, device=dev) if want_diag else None
    for lo in range(0, max(cols, 1), _lib.TWOSAMPLE_MAX_COLS):
        part = labels if cols <= _lib.TWOSAMPLE_MAX_COLS else labels[:, lo:lo + _lib.TWOSAMPLE_MAX_COLS].contiguous()
        pc = part.shape[1]
        size = lib.siggan_kernel_forms_workspace(n, pc)
        ws = torch.empty(max(size, 8) // 8, dtype=torch.float64, device=dev)
        _lib.check(lib.siggan_kernel_forms(dev.index, ptr(x), n, dim, C.byref(spec), ptr(part), pc, ptr(forms[lo:lo + pc]),
                                           ptr(diag if lo == 0 else None), ptr(ws), size, stream(dev)))
    return (forms, diag) if want_diag else forms


# ---- definitions (pure numpy) ----------------------------------------------------------------------------------------------
def mmd2_from_forms(forms, n_a: int, n_b: int) -> np.ndarray:
    """The unbiased estimator MMD^2_u = F_AA / (n_a (n_a - 1)) + F_BB / (n_b (n_b - 1)) - 2 F_AB / (n_a n_b) for every row
    (F_AA, F_BB, F_AB) of ``forms`` (sums over ORDERED pairs, the diagonal left out; ``kernel_forms``); fp64 (cols)."""
    n_a, n_b = int(n_a), int(n_b)
    if n_a < 2 or n_b < 2:
        raise ValueError(f"the unbiased estimator needs at least 2 rows per group, got {n_a} and {n_b}")
    f = np.asarray(forms, dtype=np.float64).reshape(-1, 3)
    return f[:, 0] / (n_a * (n_a - 1)) + f[:, 1] / (n_b * (n_b - 1)) - 2.0 * f[:, 2] / (n_a * n_b)


def p_value(stats) -> float:
    """(1 + #{p >= 1 : stats[p] >= stats[0]}) / (1 + permutations): stats[0] is the observed statistic, a tie counts."""
    s = np.asarray(stats, dtype=np.float64).reshape(-1)
    if s.size < 2:
        raise ValueError("a p-value needs the observed statistic and at least one permuted one")
    return float(1 + int((s[1:] >= s[0]).sum())) / float(s.size)


def _check_counts(n_real: int, n_fake: int) -> Tuple[int, int]:
    n_real, n_fake = int(n_real), int(n_fake)
    if n_real < 2 or n_fake < 2:
        raise ValueError(f"a two-sample statistic needs at least 2 rows per set, got {n_real} real and {n_fake} generated")
    if n_real + n_fake > _lib.TWOSAMPLE_MAX_N:
        raise ValueError(f"{n_real} + {n_fake} pooled rows exceed SIGGAN_TWOSAMPLE_MAX_N = {_lib.TWOSAMPLE_MAX_N}; "
                         "evaluate fewer samples")
    return n_real, n_fake


def permutation_labels(n_real: int, n_fake: int, permutations: int, seed: int) -> np.ndarray:
    """uint8 (n_real + n_fake, permutations + 1): column 0 is the observed labelling (real = 1, generated = 2), every other
    column that vector permuted by ``numpy.random.default_rng(seed)``."""
    n_real, n_fake = _check_counts(n_real, n_fake)
    permutations = int(permutations)
    if permutations < 1:
        raise ValueError(f"permutations must be >= 1, got {permutations}")
    observed = np.concatenate([np.full(n_real, 1, np.uint8), np.full(n_fake, 2, np.uint8)])
    rng = np.random.default_rng(seed)
    out = np.empty((n_real + n_fake, permutations + 1), np.uint8)
    out[:, 0] = observed
    for p in range(1, permutations + 1):
        out[:, p] = rng.permutation(observed)
    return out


def subset_labels(n_real: int, n_fake: int, subsets: int, subset_size: int, seed: int) -> np.ndarray:
    """uint8 (n_real + n_fake, subsets): per column ``subset_size`` real rows (the first n_real) carry 1 and ``subset_size``
    generated rows carry 2, drawn without replacement by ``numpy.random.default_rng(seed)``; the rest are 0."""
    n_real, n_fake = _check_counts(n_real, n_fake)
    subsets, subset_size = int(subsets), int(subset_size)
    if subsets < 1:
        raise ValueError(f"subsets must be >= 1, got {subsets}")
    if not 2 <= subset_size <= min(n_real, n_fake):
        raise ValueError(f"subset_size = {subset_size} outside [2, min(n_real, n_fake) = {min(n_real, n_fake)}]")
    rng = np.random.default_rng(seed)
    out = np.zeros((n_real + n_fake, subsets), np.uint8)
    for p in range(subsets):
        out[rng.choice(n_real, subset_size, replace=False), p] = 1
        out[n_real + rng.choice(n_fake, subset_size, replace=False), p] = 2
    return out


def median_heuristic_gamma(rows: np.ndarray) -> float:
    """1 / median of the squared distances between the distinct pairs of ``rows`` (numpy fp64)."""
    r = np.asarray(rows, dtype=np.float64)
    d2 = ((r[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(r.shape[0], 1)]
    med = float(np.median(d2))
    if not med > 0:
        raise ValueError("the median squared distance of the pooled rows is 0: no bandwidth to take from it")
    return 1.0 / med


# ---- the statistics ----------------------------------------------------------------------------------------------------------
def _pool(real_emb: torch.Tensor, fake_emb: torch.Tensor) -> torch.Tensor:
    for name, t in (("real_emb", real_emb), ("fake_emb", fake_emb)):
        check_rows(name, t, torch.float32, "(n, dim)", contiguous=False)            # torch.cat below copies anyway
    if real_emb.device != fake_emb.device or real_emb.shape[1] != fake_emb.shape[1]:
        raise ValueError(f"real_emb {tuple(real_emb.shape)} on {real_emb.device} and fake_emb {tuple(fake_emb.shape)} on "
                         f"{fake_emb.device} must share device and dim")
    _check_counts(real_emb.shape[0], fake_emb.shape[0])
    return torch.cat([real_emb, fake_emb], dim=0).contiguous()


def _forms_host(pooled: torch.Tensor, labels: np.ndarray, **kernel) -> np.ndarray:
    return kernel_forms(pooled, torch.from_numpy(labels).to(pooled.device), **kernel).cpu().numpy()


def kid_values(real_emb: torch.Tensor, fake_emb: torch.Tensor, subsets: int = 100, subset_size: Optional[int] = None,
               gamma: Optional[float] = None, seed: int = 0) -> Tuple[np.ndarray, float, int, float]:
    """(the per-subset estimates fp64 (subsets), the estimate on the full sets, subset_size, gamma) behind ``kid``: one
    ``kernel_forms`` call over subsets + 1 label columns."""
    pooled = _pool(real_emb, fake_emb)
    n_real, n_fake = real_emb.shape[0], fake_emb.shape[0]
    size = min(n_real, n_fake, KID_MAX_SUBSET) if subset_size is None else int(subset_size)
    gamma = 1.0 / pooled.shape[1] if gamma is None else float(gamma)
    labels = np.concatenate([subset_labels(n_real, n_fake, subsets, size, seed),
                             permutation_labels(n_real, n_fake, 1, 0)[:, :1]], axis=1)        # one more column: the full sets
    forms = _forms_host(pooled, labels, kind="poly", gamma=gamma, coef0=1.0, degree=3)
    return mmd2_from_forms(forms[:-1], size, size), float(mmd2_from_forms(forms[-1:], n_real, n_fake)[0]), size, gamma


def kid(real_emb: torch.Tensor, fake_emb: torch.Tensor, subsets: int = 100, subset_size: Optional[int] = None,
        gamma: Optional[float] = None, seed: int = 0) -> Dict[str, Any]:
    """Kernel Inception Distance of two (n, dim) fp32 sets on one ROCm device: the unbiased MMD^2 under the cubic polynomial
    kernel (gamma a.b + 1)^3 over ``subsets`` random subsets of ``subset_size`` rows per set (default min(n_real, n_fake,
    1000)).  -> {kid_mean, kid_std (numpy's, ddof = 0), kid_full (the estimator on the full sets), subsets, subset_size,
    gamma}.  gamma defaults to 1 / dim, the literature's value -- with unit-norm rows at dim 128 that makes the kernel almost
    linear, so KID mostly compares means; raise gamma, or use mmd_permutation_test."""
    values, full, size, gamma = kid_values(real_emb, fake_emb, subsets, subset_size, gamma, seed)
    return {"kid_mean": float(np.mean(values)), "kid_std": float(np.std(values)), "kid_full": full,
            "subsets": int(subsets), "subset_size": size, "gamma": gamma}


def permutation_stats(real_emb: torch.Tensor, fake_emb: torch.Tensor, permutations: int = 1000, kind: str = "rbf",
                      gamma: Optional[float] = None, seed: int = 0) -> Tuple[np.ndarray, float]:
    """(the unbiased MMD^2 of the observed labelling followed by those of ``permutations`` label permutations, fp64
    (permutations + 1); gamma) behind ``mmd_permutation_test``."""
    if kind not in KINDS:
        raise ValueError(f"kind must be 'rbf' or 'poly', got {kind!r}")
    pooled = _pool(real_emb, fake_emb)
    n_real, n_fake = real_emb.shape[0], fake_emb.shape[0]
    if gamma is None and kind == "rbf":
        n = pooled.shape[0]
        rows = np.sort(np.random.default_rng(seed).choice(n, MEDIAN_ROWS, replace=False)) if n > MEDIAN_ROWS else np.arange(n)
        gamma = median_heuristic_gamma(pooled[torch.from_numpy(rows).to(pooled.device)].cpu().numpy())
    elif gamma is None:
        gamma = 1.0 / pooled.shape[1]
    gamma = float(gamma)
    forms = _forms_host(pooled, permutation_labels(n_real, n_fake, permutations, seed), kind=kind, gamma=gamma, coef0=1.0, degree=3)
    return mmd2_from_forms(forms, n_real, n_fake), gamma


def mmd_permutation_test(real_emb: torch.Tensor, fake_emb: torch.Tensor, permutations: int = 1000, kind: str = "rbf",
                         gamma: Optional[float] = None, seed: int = 0) -> Dict[str, Any]:
    """Permutation test of the unbiased MMD^2 between two (n, dim) fp32 sets on one ROCm device.  -> {mmd2 (observed),
    p_value = (1 + #{permuted >= observed}) / (1 + permutations), null_mean, null_std, null_q95 (of the permuted statistics),
    permutations, kind, gamma}.  'rbf' with gamma None: the median heuristic, gamma = 1 / median squared distance over at
    most 512 pooled rows drawn with ``seed``, on the host in fp64, and reported; 'poly': the cubic kernel of ``kid``, gamma
    None = 1 / dim."""
    stats, gamma = permutation_stats(real_emb, fake_emb, permutations, kind, gamma, seed)
    null = stats[1:]
    return {"mmd2": float(stats[0]), "p_value": p_value(stats), "null_mean": float(np.mean(null)), "null_std": float(np.std(null)),
            "null_q95": float(np.quantile(null, 0.95)), "permutations": int(permutations), "kind": kind, "gamma": gamma}
