"""Elastic signature matching on the device: banded dynamic time warping (DTW) between the column profiles of byte images
(include/siggan_dtw.h, csrc/dtw.hip).

A signature is read left to right as a sequence of per-column measurements -- ink count, first and last ink row, number of
vertical runs, four bytes per column (``column_profiles``) -- and two such sequences are aligned elastically within a band
of ``band`` columns; the header states the recurrence in full.  Hand-to-hand variation is mostly local stretching and
shifting along the writing direction, which this absorbs and a pixelwise measure (ssim.py) does not.  Only that direction is
elastic: a vertical displacement is costed through the first and last ink row, on purpose, and an empty column reads as
height / 2.  Whether the distance tracks visual quality or verifier accuracy on a trained checkpoint is not measured.

The profiles of a set are made once (``DtwSet``) and every pair of two sets is scored on the device: ``dtw_matrix`` gives
all of them, ``dtw_paired`` a_i against b_i, ``dtw_best`` each row's lowest distance and its column without forming a matrix
anywhere.  All of them take contiguous uint8 device tensors (N, H, W) or (N, 1, H, W) with N >= 1, 1 <= H <= 128 and W a
multiple of 4 in 4..128, or ``DtwSet``s of them, work on the current stream and never synchronise the host.  Arguments are
validated before the library is touched; there is no CPU path.  Everything is integer arithmetic: equal input gives equal
output, DTW(x, x) is 0, DTW(a, b) and DTW(b, a) are the same integer, and a pair's value does not depend on the batch it
stands in.

``dtw_diversity`` and ``nearest_real_from_best`` are the numpy reductions of ready results: what the evaluation reports."""
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _call, _lib
from ._call import as_int, ptr, stream
from ._image_pairs import CLOSEST, LPIPS_IMAGES, LPIPS_REACH, PAIRED, host, mode, nearest_real, outputs, pair_sets  # noqa: F401


def default_band(w: int) -> int:
    """max(1, w // 8) columns: 8 at 64, 16 at 128."""
    return max(1, int(w) // 8)


def check_threshold(threshold) -> int:
    threshold = as_int(threshold, "threshold")
    if not 1 <= threshold <= 255:
        raise ValueError(f"threshold = {threshold} outside [1, 255]")
    return threshold


def check_band(band, w: int) -> int:
    """``band`` None: default_band(w).  0 <= band <= w - 1."""
    band = default_band(w) if band is None else as_int(band, "band")
    if not 0 <= band <= w - 1:
        raise ValueError(f"band = {band} outside [0, {w - 1}]")
    return band


def check_shape(u8, what: str = "images") -> Tuple[int, int, int]:
    """The refusals of the images that need no device: type, dtype, rank, sizes.  Returns (n, h, w)."""
    return _call.check_u8_images(u8, what, 1, 4, _lib.DTW_MAX_SIZE, False, kinds="a tensor or a DtwSet")


def _profiles(u8: torch.Tensor, n: int, h: int, w: int, threshold: int) -> torch.Tensor:
    out = torch.empty((n, w, 4), dtype=torch.uint8, device=u8.device)
    _lib.check(_lib.load().siggan_dtw_profiles_u8(_call.device_of(u8).index, ptr(u8), n, h, w, threshold, ptr(out), stream(u8.device)))
    return out


def column_profiles(u8: torch.Tensor, threshold: int = 128) -> torch.Tensor:
    """uint8 (N, W, 4) on the device: per column the ink count, the first and the last ink row (H // 2 for a column without
    ink) and the number of vertical ink runs; ink is byte < ``threshold``.  The four bytes are one little-endian dword."""
    n, h, w = check_shape(u8)
    threshold = check_threshold(threshold)
    _call.check_resident(u8, "images")
    return _profiles(u8, n, h, w, threshold)


class DtwSet:
    """The column profiles of a set of byte images (uint8 (N, W, 4)), made once: a set is profiled once however many sets it
    is later compared with.  The bytes themselves are not kept.  Sets that are compared share the width and the device; the
    HEIGHTS may differ (rows are absolute: a taller image's ink simply reaches further down)."""

    def __init__(self, u8: torch.Tensor, threshold: int = 128) -> None:
        self.n, self.h, self.w = check_shape(u8)
        self.threshold = check_threshold(threshold)
        _call.check_resident(u8, "images")
        self.device = _call.device_of(u8)
        self.profiles = _profiles(u8, self.n, self.h, self.w, self.threshold)

    def __len__(self) -> int:
        return self.n

    def first(self, count: int) -> "DtwSet":
        """The set of the first ``count`` images (at least one), sharing their profiles."""
        head = object.__new__(DtwSet)
        head.__dict__.update(self.__dict__)
        head.n = max(1, min(int(count), self.n))
        head.profiles = self.profiles[:head.n]
        return head


Images = Union[torch.Tensor, DtwSet]


def _two(a: Images, b: Optional[Images], band, paired: bool = False) -> Tuple[DtwSet, Optional[DtwSet], int]:
    """Both sides validated (a first), then the band, then where they live -- before either is profiled."""
    shapes = []
    for x, what in ((a, "a"), (b, "b")):
        if x is None and what == "b" and not paired:
            continue
        shapes.append((x.n, x.w) if isinstance(x, DtwSet) else check_shape(x, what)[::2])
    if len(shapes) == 2:
        if shapes[0][1] != shapes[1][1]:
            raise ValueError(f"a is {shapes[0][1]} columns wide and b {shapes[1][1]}: DTW compares profiles of equal width")
        if paired and shapes[0][0] != shapes[1][0]:
            raise ValueError(f"a holds {shapes[0][0]} images and b {shapes[1][0]}: paired DTW needs equally many")
    band = check_band(band, shapes[0][1])
    for x, what in ((a, "a"), (b, "b")):
        if isinstance(x, torch.Tensor):
            _call.check_resident(x, what)
    a = a if isinstance(a, DtwSet) else DtwSet(a)
    if b is None:
        return a, None, band
    b = b if isinstance(b, DtwSet) else DtwSet(b)
    if a.device != b.device:
        raise ValueError(f"a lives on {a.device} and b on {b.device}")
    return a, b, band


def _pairs(a: DtwSet, b: Optional[DtwSet], band: int, mode: int, matrix=None, best=None, index=None) -> None:
    b_prof, nb = (b.profiles, b.n) if b is not None else (None, a.n)                     # SAME_SET: b is a
    _lib.check(_lib.load().siggan_dtw_pairs(a.device.index, ptr(a.profiles), a.n, ptr(b_prof), nb, a.w, band, mode, ptr(matrix),
                                            ptr(best), ptr(index), stream(a.device)))


def _scored(a: Images, b: Optional[Images], band, matrix: bool, best: bool):
    a, b, band = _two(a, b, band)
    out = outputs(a, b, torch.int32, matrix, best)
    _pairs(a, b, band, mode(b), *out)
    return out


def dtw_matrix(a: Images, b: Optional[Images] = None, band: Optional[int] = None) -> torch.Tensor:
    """int32 (len(a), len(b)) on the device: the DTW distance of every a_i to every b_j within ``band`` columns (None:
    default_band(W)).  ``b`` None: a against itself, (n, n), symmetric with a diagonal of 0."""
    return _scored(a, b, band, True, False)[0]


def dtw_paired(a: Images, b: Images, band: Optional[int] = None) -> torch.Tensor:
    """int32 (n,) on the device: DTW(a_i, b_i); the two sets hold equally many images."""
    if b is None:
        raise ValueError("b must be a tensor or a DtwSet, got NoneType")
    a, b, band = _two(a, b, band, paired=True)
    out = torch.empty((a.n,), dtype=torch.int32, device=a.device)
    _pairs(a, b, band, PAIRED, matrix=out)
    return out


def dtw_best(a: Images, b: Optional[Images] = None, band: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(int32 (len(a),), int32 (len(a),)) on the device: each a_i's lowest distance to an image of ``b`` and that image's
    index, equal values resolved to the lower index.  ``b`` None: to another image of ``a`` itself (j = i is left out; a
    single image gives -1 / -1).  No matrix is formed."""
    return _scored(a, b, band, False, True)[1:]


def dtw_matrix_and_best(a: Images, b: Optional[Images] = None, band: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dtw_matrix, *dtw_best) of the same arguments out of one launch; the integers are those of the separate calls."""
    return _scored(a, b, band, True, True)


# ---- numpy reductions of ready results ----------------------------------------------------------------------------------
def _width(w) -> int:
    w = as_int(w, "w")
    if w < 1:
        raise ValueError(f"w = {w} < 1")
    return w


def _pair_set(values: np.ndarray, w: int) -> Dict[str, Any]:
    if values.size == 0:
        return {"pairs": 0, "mean_distance": None, "diversity": None}
    mean = float(np.mean(values))
    return {"pairs": int(values.size), "mean_distance": mean, "diversity": mean / w}


def dtw_diversity(matrix, w: int) -> Dict[str, Any]:
    """Mean pairwise DTW distance of a set from its own (n, n) matrix, and ``diversity`` = that mean per column (divided by
    the width ``w``): higher means more diverse, the direction of LPIPS.  Two pair sets: ``lpips_pairs``, the reference's
    LPIPS pair set (i < j < i + 10 over the first min(100, n) images), and ``all_pairs``, the full upper triangle.  A set of
    one image has no pair: means are None."""
    w = _width(w)
    n, near, every = pair_sets(matrix)
    return {"n": n, "w": w, "lpips_pairs": _pair_set(near, w), "all_pairs": _pair_set(every, w)}


def nearest_real_from_best(best, index, real_loo_best, w: int) -> Dict[str, Any]:
    """Each generated image's lowest distance to a real one (``best`` / ``index`` of dtw_best(generated, real)) against the
    real set's own leave-one-out values (``best`` of dtw_best(real); None or empty for a real set of one image), all PER
    COLUMN (the integer distance divided by the width ``w``).  mean / median / min; real_loo_median; excess_median =
    real_loo_median - median, where a clearly positive value says the generated images sit closer to a real one than the
    real ones sit to each other: the memorisation warning; closest: the five (generated index, real index, distance per
    column) of lowest distance, equal values by generated index."""
    w = _width(w)
    loo = host(real_loo_best, np.float64).reshape(-1) / w if real_loo_best is not None else np.zeros(0)
    return nearest_real(host(best, np.int64).reshape(-1).astype(np.float64) / w, host(index, np.int64).reshape(-1), loo,
                        higher_is_closer=False)
