"""Mode counting between two sets of feature vectors that stay on the device: k-means bins, the number of statistically
different bins (NDB) and the Jensen-Shannon divergence of the bin histograms (Richardson & Weiss 2018).

Coverage (utils/neighbors.py) counts real samples that have a generated sample in their k-NN ball; it says nothing about
proportions.  Here the real set is clustered into K bins, every generated row goes to its nearest bin, and a two-proportion
z-test says, bin by bin, whether the Generator produces that group too rarely, too often or not at all.

``kmeans`` and ``assign`` (include/siggan_kmeans.h, csrc/kmeans.hip) run k-means++ seeding and Lloyd passes in fp64 on the
device: fixed-order sums, so equal input gives equal bits; the assignment is ``knn`` with k = 1, bit for bit.
``ndb_from_counts`` -- pure numpy and math, the definitions in one place -- turns two histograms into the report;
``mode_coverage`` puts them together and carries the real set's own noise floor (a held-out half of the real rows against
the bins of the other half), in the way ``nearest_real`` carries the real set's leave-one-out values.

Whether NDB on these features tracks visual quality on a trained checkpoint is not measured here."""
import math
from typing import Any, Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _call, _lib
from .._call import ptr, stream
from .neighbors import knn

UNDER_REPRESENTED = 5                                       # how many bins ``most_under_represented`` lists


class KMeansResult(NamedTuple):
    centres: torch.Tensor            # (k, dim) fp32
    labels: torch.Tensor             # (n,) int32
    counts: torch.Tensor             # (k,) int32
    mind2: torch.Tensor              # (n,) fp64: squared distance to the row's centre
    inertia: torch.Tensor            # (iterations + 1,) fp64, per pass
    changed: torch.Tensor            # (iterations + 1,) int32, per pass
    seed_rows: torch.Tensor          # (k,) int32: the rows the seeding chose
    restart: int                     # which restart won
    empty_clusters: int              # centres without a row


def _check_rows(name: str, x) -> torch.device:
    _call.check_rows(name, x, torch.float32, "(n >= 1, dim)", min_rows=1)
    n, dim = x.shape
    if n > _lib.KMEANS_MAX_N:
        raise ValueError(f"{name} has {n} rows, at most {_lib.KMEANS_MAX_N} are supported")
    if not 1 <= dim <= _lib.KMEANS_MAX_DIM:
        raise ValueError(f"dim = {dim} outside [1, {_lib.KMEANS_MAX_DIM}]")
    return _call.device_of(x)


def _workspace(lib, n: int, dim: int, k: int, dev: torch.device) -> Tuple[torch.Tensor, int]:
    size = int(lib.siggan_kmeans_workspace(n, dim, k))
    return torch.empty(max(size, 8) // 8, dtype=torch.float64, device=dev), size


def _lloyd(lib, x, centres, iterations, dev, workspace, size):
    n, dim = x.shape
    k = centres.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    mind2 = torch.empty(n, dtype=torch.float64, device=dev)
    counts = torch.empty(k, dtype=torch.int32, device=dev)
    inertia = torch.empty(iterations + 1, dtype=torch.float64, device=dev)
    changed = torch.empty(iterations + 1, dtype=torch.int32, device=dev)
    _lib.check(lib.siggan_kmeans_lloyd(dev.index, ptr(x), n, dim, ptr(centres), k, iterations, ptr(labels), ptr(mind2), ptr(counts),
                                       ptr(inertia), ptr(changed), ptr(workspace), size, stream(dev)))
    return labels, mind2, counts, inertia, changed


def seed_centres(x: torch.Tensor, k: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(centres fp32 (k, dim), seed_rows int32 (k,)): k-means++ seeding of the rows of x (n, dim) fp32 on a ROCm device
    (siggan_kmeans_seed; the header states the draw and the sampling rule).  Nothing synchronises the host."""
    dev = _check_rows("x", x)
    n, dim = x.shape
    k = _check_k(k, n)
    seed = _check_seed(seed)
    lib = _lib.load()
    workspace, size = _workspace(lib, n, dim, k, dev)
    centres = torch.empty(k, dim, dtype=torch.float32, device=dev)
    rows = torch.empty(k, dtype=torch.int32, device=dev)
    _lib.check(lib.siggan_kmeans_seed(dev.index, ptr(x), n, dim, k, seed, ptr(centres), ptr(rows), ptr(workspace), size, stream(dev)))
    return centres, rows


def _check_k(k, n: int) -> int:
    k = _call.as_int(k, "k")
    if not 1 <= k <= min(n, _lib.KMEANS_MAX_K):
        raise ValueError(f"k = {k} outside [1, min(n = {n}, {_lib.KMEANS_MAX_K})]")
    return k


def _check_seed(seed) -> int:
    seed = _call.as_int(seed, "seed")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"seed = {seed} outside [0, 2^64)")
    return seed


def kmeans(x: torch.Tensor, k: int, iterations: int = 50, restarts: int = 4, seed: int = 0) -> KMeansResult:
    """k-means of the rows of x (n, dim) fp32 on a ROCm device: ``restarts`` runs of k-means++ seeding (restart r seeds with
    ``seed + r``) and ``iterations`` Lloyd passes each.  All restarts are enqueued, then ONE host read of their final inertias
    picks the lowest, equal ones by the lower r.  The returned labels, distances and counts belong to the returned centres.
    1 <= k <= min(n, 256), n <= 65536, dim <= 1024, 0 <= iterations <= 1000, restarts >= 1."""
    dev = _check_rows("x", x)
    n, dim = x.shape
    k = _check_k(k, n)
    iterations = _call.as_int(iterations, "iterations")
    if not 0 <= iterations <= _lib.KMEANS_MAX_ITERATIONS:
        raise ValueError(f"iterations = {iterations} outside [0, {_lib.KMEANS_MAX_ITERATIONS}]")
    restarts = _call.as_int(restarts, "restarts")
    if restarts < 1:
        raise ValueError(f"restarts must be >= 1, got {restarts}")
    seed = _check_seed(seed)
    lib = _lib.load()
    workspace, size = _workspace(lib, n, dim, k, dev)       # one stream: the runs follow each other and may share it
    runs = []
    for r in range(restarts):
        centres = torch.empty(k, dim, dtype=torch.float32, device=dev)
        rows = torch.empty(k, dtype=torch.int32, device=dev)
        _lib.check(lib.siggan_kmeans_seed(dev.index, ptr(x), n, dim, k, (seed + r) & ((1 << 64) - 1), ptr(centres), ptr(rows),
                                          ptr(workspace), size, stream(dev)))
        runs.append((centres, rows) + _lloyd(lib, x, centres, iterations, dev, workspace, size))
    # the one host read: every run's final inertia and its number of empty clusters
    final = torch.stack([torch.stack([run[5][iterations], (run[4] == 0).sum().to(torch.float64)]) for run in runs]).cpu().numpy()
    best = int(np.argmin(final[:, 0]))                                               # the first of equal minima
    centres, rows, labels, mind2, counts, inertia, changed = runs[best]
    return KMeansResult(centres, labels, counts, mind2, inertia, changed, rows, best, int(final[best, 1]))


def assign(x: torch.Tensor, centres: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(labels int32 (n,), mind2 fp64 (n,), counts int32 (k,)): every row of x into its nearest of the given centres (k, dim)
    fp32 -- the iterations = 0 call, which reads the centres in place and leaves them untouched.  Equal distances go to the
    lower centre; labels and mind2 are knn(x, centres, 1)'s, bit for bit."""
    dev = _check_rows("x", x)
    n, dim = x.shape
    _call.check_rows("centres", centres, torch.float32, f"(1 <= k <= {_lib.KMEANS_MAX_K}, {dim})", shape=(None, dim), min_rows=1,
                     device=x.device, where=str(x.device))
    k = centres.shape[0]
    if k > _lib.KMEANS_MAX_K:
        raise ValueError(f"centres holds {k} rows, at most {_lib.KMEANS_MAX_K} are supported")
    if k > n:
        raise ValueError(f"centres holds k = {k} rows, more than the n = {n} rows of x: the call takes k <= n")
    lib = _lib.load()
    workspace, size = _workspace(lib, n, dim, k, dev)
    labels, mind2, counts, _, _ = _lloyd(lib, x, centres, 0, dev, workspace, size)
    return labels, mind2, counts


def pixel_features(u8: torch.Tensor, factor: int = 4) -> torch.Tensor:
    """fp32 rows (N, (S / factor)^2) of ``factor`` x ``factor`` box means of byte images (N, S, S) or (N, 1, S, S): 256
    features at 64 x 64 and 1024 at 128 x 128 with factor 4.  Torch ops on the tensor's own device; a sum of factor^2 bytes
    divided by a power of two is exact in fp32, so the rows do not depend on the order of anything."""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8:
        raise ValueError(f"images must be a torch.uint8 tensor, got {getattr(u8, 'dtype', type(u8).__name__)}")
    if not (u8.dim() == 3 or (u8.dim() == 4 and u8.shape[1] == 1)) or u8.shape[-1] != u8.shape[-2]:
        raise ValueError(f"images must be (N, S, S) or (N, 1, S, S), got {tuple(u8.shape)}")
    factor = _call.as_int(factor, "factor")
    side = u8.shape[-1]
    if factor < 1 or factor & (factor - 1) or side % factor:
        raise ValueError(f"factor = {factor} must be a power of two that divides the side {side}")
    cells = side // factor
    sums = u8.reshape(-1, cells, factor, cells, factor).to(torch.int32).sum(dim=(2, 4))
    return (sums.to(torch.float32) / float(factor * factor)).reshape(-1, cells * cells).contiguous()


def ndb_from_counts(ref_counts, test_counts, alpha: float = 0.05) -> Dict[str, Any]:
    """The number of statistically different bins between a reference histogram r and a test histogram t over the same K
    bins (numpy and math, no device).  With N_r, N_t the totals, p_j = r_j / N_r, q_j = t_j / N_t and the pooled proportion
    P_j = (r_j + t_j) / (N_r + N_t):  z_j = (p_j - q_j) / sqrt(P_j (1 - P_j) (1 / N_r + 1 / N_t)), 0 where the denominator
    is 0; the two-sided p-value is erfc(|z_j| / sqrt 2); a bin is different when p < alpha.

    Keys: k, n_ref, n_test, alpha, ndb, ndb_over_k, js_divergence (base 2, 0 log 0 = 0: in [0, 1]), z, different_bins,
    missing_bins (t_j = 0 < r_j) and most_under_represented (up to five bins by the most positive z: [bin, z, r_j, t_j])."""
    r = np.asarray(ref_counts).reshape(-1)
    t = np.asarray(test_counts).reshape(-1)
    if r.size < 1 or r.size != t.size:
        raise ValueError(f"ref_counts ({r.size}) and test_counts ({t.size}) must hold the same K >= 1 bins")
    if not (np.issubdtype(r.dtype, np.integer) and np.issubdtype(t.dtype, np.integer)) or r.min() < 0 or t.min() < 0:
        raise ValueError("counts must be non-negative integers")
    alpha = float(alpha)
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha must be in (0, 1), got {alpha}")
    r, t = r.astype(np.int64), t.astype(np.int64)
    n_r, n_t = int(r.sum()), int(t.sum())
    if n_r < 1 or n_t < 1:
        raise ValueError(f"both histograms must hold a sample, got {n_r} and {n_t}")
    p, q = r / n_r, t / n_t
    pooled = (r + t) / (n_r + n_t)
    denom = np.sqrt(pooled * (1.0 - pooled) * (1.0 / n_r + 1.0 / n_t))
    z = np.divide(p - q, denom, out=np.zeros(r.size), where=denom > 0)
    p_value = np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z])
    different = np.flatnonzero(p_value < alpha)
    mid = 0.5 * (p + q)

    def kl(a):                                               # sum a log2(a / mid), 0 log 0 = 0; mid > 0 wherever a > 0
        on = a > 0
        return float(np.sum(a[on] * np.log2(a[on] / mid[on])))

    js = min(1.0, max(0.0, 0.5 * kl(p) + 0.5 * kl(q)))
    under = np.lexsort((np.arange(r.size), -z))[:UNDER_REPRESENTED]                  # by z descending, equal ones by bin
    return {"k": int(r.size), "n_ref": n_r, "n_test": n_t, "alpha": alpha, "ndb": int(different.size),
            "ndb_over_k": float(different.size) / r.size, "js_divergence": js, "z": [float(v) for v in z],
            "different_bins": [int(j) for j in different], "missing_bins": [int(j) for j in np.flatnonzero((t == 0) & (r > 0))],
            "most_under_represented": [[int(j), float(z[j]), int(r[j]), int(t[j])] for j in under if z[j] > 0]}


def default_k(n_bins_rows: int) -> int:
    """K when the caller names none: about 20 rows per bin, between 2 and 100."""
    return max(2, min(100, n_bins_rows // 20))


def mode_coverage(real_feats: torch.Tensor, fake_feats: torch.Tensor, k: Optional[int] = None, seed: int = 0, alpha: float = 0.05,
                  iterations: int = 50, restarts: int = 4) -> Dict[str, Any]:
    """NDB and JS divergence of generated rows against real rows, both (n, dim) fp32 on one ROCm device.

    A host permutation (numpy default_rng(seed)) splits the real rows into halves A (the first ceil(n / 2) of the permutation)
    and B.  Bins are kmeans(A).  ``generated_vs_real`` = ndb_from_counts(A's counts, assign(fake)); ``real_holdout_vs_real`` =
    ndb_from_counts(A's counts, assign(B)), the noise floor: what two samples of the SAME distribution show.  With fewer than
    2 k rows in B the floor is None and ``real_holdout_reason`` says why.  ``k`` None: default_k(len(A)).

    Further keys: k, n_bins_rows, n_holdout_rows, n_generated, seed, iterations, restarts, restart, final_inertia,
    converged_at (the pass at which ``changed`` reached 0, or None), empty_clusters (the bins without a row of A) and
    under_represented_examples: for each of generated_vs_real's most under-represented bins, the row of real_feats nearest
    to its centre (knn(centres, A, 1)) and its distance, so a user can look at what is missing."""
    dev = _check_rows("real_feats", real_feats)
    _check_rows("fake_feats", fake_feats)
    if fake_feats.device != real_feats.device or fake_feats.shape[1] != real_feats.shape[1]:
        raise ValueError(f"real_feats {tuple(real_feats.shape)} on {real_feats.device} and fake_feats {tuple(fake_feats.shape)} on "
                         f"{fake_feats.device} must share device and dim")
    n_real = real_feats.shape[0]
    if n_real < 4:
        raise ValueError(f"mode_coverage needs at least 4 real rows to split, got {n_real}")
    seed = _check_seed(seed)
    perm = np.random.default_rng(seed).permutation(n_real)
    n_a = (n_real + 1) // 2
    index = torch.from_numpy(perm.astype(np.int64)).to(dev)
    a_rows, b_rows = real_feats[index[:n_a]].contiguous(), real_feats[index[n_a:]].contiguous()
    k = default_k(n_a) if k is None else _check_k(k, n_a)
    if fake_feats.shape[0] < k:
        raise ValueError(f"fake_feats has {fake_feats.shape[0]} rows, fewer than the k = {k} bins")
    bins = kmeans(a_rows, k, iterations, restarts, seed)
    _, _, fake_counts = assign(fake_feats, bins.centres)
    ref = bins.counts.cpu().numpy()
    generated = ndb_from_counts(ref, fake_counts.cpu().numpy(), alpha)
    holdout, reason = None, None
    if b_rows.shape[0] < 2 * k:
        reason = f"the held-out half has {b_rows.shape[0]} rows, fewer than 2 k = {2 * k}"
    else:
        holdout = ndb_from_counts(ref, assign(b_rows, bins.centres)[2].cpu().numpy(), alpha)
    changed = bins.changed.cpu().numpy()
    still = np.flatnonzero(changed == 0)
    examples = []
    if generated["most_under_represented"]:
        d2, nearest = knn(bins.centres, a_rows, 1)
        d2, nearest = d2.cpu().numpy()[:, 0], nearest.cpu().numpy()[:, 0]
        examples = [{"bin": j, "real_row": int(perm[nearest[j]]), "distance": float(math.sqrt(d2[j]))}
                    for j, _, _, _ in generated["most_under_represented"]]
    return {"k": k, "n_bins_rows": n_a, "n_holdout_rows": int(b_rows.shape[0]), "n_generated": int(fake_feats.shape[0]),
            "seed": seed, "iterations": int(iterations), "restarts": int(restarts), "restart": bins.restart,
            "final_inertia": float(bins.inertia[-1].item()), "converged_at": int(still[0]) if still.size else None,
            "empty_clusters": [int(j) for j in np.flatnonzero(ref == 0)],
            "generated_vs_real": generated, "real_holdout_vs_real": holdout, "real_holdout_reason": reason,
            "under_represented_examples": examples}

