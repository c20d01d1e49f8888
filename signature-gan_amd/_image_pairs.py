"""What the wrappers of the ops that score every image of a set ``a`` against every image of a set ``b`` share (ssim.py,
dtw.py; csrc/image_pairs.h on the other side of the ABI): the mode and the outputs of a call, and the numpy reductions of
ready results that the evaluation reports.  Plain functions.  A measure is "higher is closer" (SSIM) or "lower is closer"
(DTW), which is one boolean; an op's key names, its scaling and the refusals of its own arguments stay in its module."""
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib

ALL, SAME_SET, PAIRED = 0, 1, 2
assert (_lib.SSIM_ALL, _lib.SSIM_SAME_SET, _lib.SSIM_PAIRED) == (_lib.DTW_ALL, _lib.DTW_SAME_SET, _lib.DTW_PAIRED) == (ALL, SAME_SET, PAIRED)
LPIPS_IMAGES, LPIPS_REACH, CLOSEST = 100, 10, 5    # the reference's LPIPS pair set: i < j < i + 10 over the first 100 images; the closest listed


def mode(b) -> int:                         # ``b`` None: a against itself
    return ALL if b is not None else SAME_SET


def outputs(a, b, dtype: torch.dtype, matrix: bool = False, best: bool = False) -> Tuple[Optional[torch.Tensor], ...]:
    """(matrix, best, index) of a call on the sets ``a`` and ``b`` (None: a itself), None where not wanted: ``dtype``
    (len(a), len(b)), ``dtype`` (len(a),), int32 (len(a),), on a's device."""
    new = lambda want, shape, kind: torch.empty(shape, dtype=kind, device=a.device) if want else None       # noqa: E731
    return new(matrix, (a.n, b.n if b is not None else a.n), dtype), new(best, (a.n,), dtype), new(best, (a.n,), torch.int32)


def host(x, dtype) -> np.ndarray:
    return np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=dtype)


def pair_sets(matrix) -> Tuple[int, np.ndarray, np.ndarray]:
    """(n, near, every) of a set's own (n, n) matrix, as float64: the values of the reference's LPIPS pair set (i < j < i + 10
    over the first min(100, n) images) and of the full upper triangle."""
    m = host(matrix, np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError(f"matrix must be (n, n) with n >= 1, got {m.shape}")
    n = m.shape[0]
    first = min(LPIPS_IMAGES, n)
    near = [m[i, j] for i in range(first) for j in range(i + 1, min(i + LPIPS_REACH, first))]
    return n, np.asarray(near, dtype=np.float64), m[np.triu_indices(n, 1)]


def nearest_real(best: np.ndarray, index: np.ndarray, loo: np.ndarray, higher_is_closer: bool) -> Dict[str, Any]:
    """The summary both ``nearest_real_from_best`` give, of float64 ``best`` / its ``index`` and the real set's leave-one-out ``loo``
    (possibly empty): the closest value of all is "max" or "min", excess_median is positive where generated images sit closer."""
    if best.size < 1 or best.size != index.size:
        raise ValueError(f"best has {best.size} entries and index {index.size}: need equally many, at least one")
    median = float(np.median(best))
    loo_median = float(np.median(loo)) if loo.size else None
    order = np.lexsort((np.arange(best.size), -best if higher_is_closer else best))[:CLOSEST]
    return {"n_generated": int(best.size), "n_real_loo": int(loo.size), "mean": float(np.mean(best)), "median": median,
            **({"max": float(np.max(best))} if higher_is_closer else {"min": float(np.min(best))}), "real_loo_median": loo_median,
            "excess_median": (median - loo_median if higher_is_closer else loo_median - median) if loo_median is not None else None,
            "closest": [(int(i), int(index[i]), float(best[i])) for i in order]}
