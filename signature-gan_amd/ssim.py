"""Structural similarity (SSIM) between byte images on the device (include/siggan_ssim.h, csrc/ssim.hip).

Single scale, L = 255, an 11-tap Gaussian window of sigma 1.5 applied at valid positions only -- the definition of Wang et al.
(2004) in fp32; the header states it in full.  The means and variances of an image are prepared once (``SsimSet``), a pair
costs one filtered product, and every pair of two sets is scored on the device: ``ssim_matrix`` gives all of them,
``ssim_paired`` a_i against b_i, ``ssim_best`` each row's highest value and its column without forming a matrix anywhere.

All of them take contiguous uint8 device tensors (N, H, W) or (N, 1, H, W) with N >= 1, 11 <= H <= 128 and W a multiple of 4
in 12..128, or ``SsimSet``s of them, work on the current stream and never synchronise the host.  Arguments are validated
before the library is touched; there is no CPU path.  Equal input gives bit-equal output: SSIM(x, x) is exactly 1.0,
SSIM(x, y) and SSIM(y, x) are the same bits, and a pair's value does not depend on the batch it stands in.

``ssim_diversity`` and ``nearest_real_from_best`` are the numpy reductions of ready results: what the evaluation reports."""
import ctypes as C
from typing import Any, Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _call, _lib
from ._call import ptr, stream
from ._image_pairs import CLOSEST, LPIPS_IMAGES, LPIPS_REACH, PAIRED, host, mode, nearest_real, outputs, pair_sets  # noqa: F401

WINDOW_TAPS, WINDOW_SIGMA = _lib.SSIM_TAPS, _lib.SSIM_SIGMA


def window() -> np.ndarray:
    """float32 (11,): the taps as the kernels use them (siggan_ssim_window; needs no device)."""
    buf = (C.c_float * WINDOW_TAPS)()
    _lib.check(_lib.load().siggan_ssim_window(buf))
    return np.frombuffer(buf, dtype=np.float32).copy()


def check_images(u8, what: str = "images") -> Tuple[int, int, int]:
    """The refusals that need no device, in a fixed order: type, dtype, rank, sizes, device, layout.  Returns (n, h, w)."""
    n, h, w = _call.check_u8_images(u8, what, _lib.SSIM_MIN_HEIGHT, _lib.SSIM_MIN_WIDTH, _lib.SSIM_MAX_SIZE, False,
                                    kinds="a tensor or an SsimSet")
    _call.check_resident(u8, what)
    return n, h, w


class SsimSet:
    """Bytes and their prepared maps (mu and variance, fp32 (N, 2, H - 10, W - 10)), made once: a set is prepared once however
    many sets it is later compared with.  The bytes are referenced, not copied: do not change them afterwards."""

    def __init__(self, u8: torch.Tensor) -> None:
        self.n, self.h, self.w = check_images(u8)
        self.u8 = u8
        self.device = _call.device_of(u8)
        self.maps = torch.empty((self.n, 2, self.h - 10, self.w - 10), dtype=torch.float32, device=u8.device)
        _lib.check(_lib.load().siggan_ssim_prepare_u8(self.device.index, ptr(u8), self.n, self.h, self.w, ptr(self.maps),
                                                      stream(u8.device)))

    def __len__(self) -> int:
        return self.n


Images = Union[torch.Tensor, SsimSet]


def _as_set(x: Images, what: str) -> SsimSet:
    if isinstance(x, SsimSet):
        return x
    check_images(x, what)
    return SsimSet(x)


def _two(a: Images, b: Optional[Images]) -> Tuple[SsimSet, Optional[SsimSet]]:
    """Both sides validated (a first) before either is prepared."""
    if not isinstance(a, SsimSet):
        check_images(a, "a")
    if b is not None and not isinstance(b, SsimSet):
        check_images(b, "b")
    a = _as_set(a, "a")
    if b is None:
        return a, None
    b = _as_set(b, "b")
    if (a.h, a.w) != (b.h, b.w):
        raise ValueError(f"a is {a.h} x {a.w} and b is {b.h} x {b.w}: SSIM compares images of equal size")
    if a.device != b.device:
        raise ValueError(f"a lives on {a.device} and b on {b.device}")
    return a, b


def _pairs(a: SsimSet, b: Optional[SsimSet], mode: int, matrix=None, best=None, index=None) -> None:
    b_u8, b_maps, nb = (b.u8, b.maps, b.n) if b is not None else (None, None, a.n)     # SAME_SET: b is a
    _lib.check(_lib.load().siggan_ssim_pairs(a.device.index, ptr(a.u8), ptr(a.maps), a.n, ptr(b_u8), ptr(b_maps), nb, a.h, a.w,
                                             mode, ptr(matrix), ptr(best), ptr(index), stream(a.device)))


def _scored(a: Images, b: Optional[Images], matrix: bool, best: bool):
    a, b = _two(a, b)
    out = outputs(a, b, torch.float32, matrix, best)
    _pairs(a, b, mode(b), *out)
    return out


def ssim_matrix(a: Images, b: Optional[Images] = None) -> torch.Tensor:
    """fp32 (len(a), len(b)) on the device: SSIM of every a_i with every b_j.  ``b`` None: a against itself, (n, n) with a
    diagonal of exactly 1.0."""
    return _scored(a, b, True, False)[0]


def ssim_paired(a: Images, b: Images) -> torch.Tensor:
    """fp32 (n,) on the device: SSIM(a_i, b_i); the two sets hold equally many images."""
    if b is None:
        raise ValueError("b must be a tensor or an SsimSet, got NoneType")
    a, b = _two(a, b)
    if a.n != b.n:
        raise ValueError(f"a holds {a.n} images and b {b.n}: paired SSIM needs equally many")
    out = torch.empty((a.n,), dtype=torch.float32, device=a.device)
    _pairs(a, b, PAIRED, matrix=out)
    return out


def ssim_best(a: Images, b: Optional[Images] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(fp32 (len(a),), int32 (len(a),)) on the device: each a_i's highest SSIM to an image of ``b`` and that image's index,
    equal values resolved to the lower index.  ``b`` None: to another image of ``a`` itself (j = i is left out; a single image
    gives -1.0 / -1).  No matrix is formed."""
    return _scored(a, b, False, True)[1:]


def ssim_matrix_and_best(a: Images, b: Optional[Images] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ssim_matrix, *ssim_best) of the same arguments out of one launch; the bits are those of the separate calls."""
    return _scored(a, b, True, True)


# ---- numpy reductions of ready results ----------------------------------------------------------------------------------
def _pair_set(values: np.ndarray) -> Dict[str, Any]:
    if values.size == 0:
        return {"pairs": 0, "mean_ssim": None, "diversity": None}
    mean = float(np.mean(values))
    return {"pairs": int(values.size), "mean_ssim": mean, "diversity": 1.0 - mean}


def ssim_diversity(matrix) -> Dict[str, Any]:
    """Mean pairwise SSIM of a set from its own (n, n) matrix, and ``diversity`` = 1 - mean: higher means more diverse, the
    direction of LPIPS.  Two pair sets: ``lpips_pairs``, the reference's LPIPS pair set (i < j < i + 10 over the first
    min(100, n) images), and ``all_pairs``, the full upper triangle.  A set of one image has no pair: means are None."""
    n, near, every = pair_sets(matrix)
    return {"n": n, "lpips_pairs": _pair_set(near), "all_pairs": _pair_set(every)}


def nearest_real_from_best(best, index, real_loo_best=None) -> Dict[str, Any]:
    """Each generated image's highest SSIM to a real one (``best`` / ``index`` of ssim_best(generated, real)) against the real
    set's own leave-one-out values (``best`` of ssim_best(real); None or empty for a real set of one image).
    mean / median / max; real_loo_median; excess_median = median - real_loo_median, where a clearly positive value says the
    generated images sit closer to a real one than the real ones sit to each other: the memorisation warning; closest: the
    five (generated index, real index, SSIM) of highest SSIM, equal values by generated index."""
    loo = host(real_loo_best, np.float64).reshape(-1) if real_loo_best is not None else np.zeros(0)
    return nearest_real(host(best, np.float64).reshape(-1), host(index, np.int64).reshape(-1), loo, higher_is_closer=True)
