"""Connected ink components of byte images on the device (include/siggan_components.h, csrc/components.hip).

A count of ink pixels cannot tell a pen line from a cloud of dots.  ``component_stats`` gives, per image, the number of ink
components, the largest one, how many components are smaller than ``min_area`` pixels and how much ink they hold, and the
bounding box of the rest; ``component_roots`` the label map (every ink pixel carries the smallest linear index of its
component, background -1); ``despeckle_u8`` a copy in which every pixel of a small component is ``fill`` and every other byte
is untouched.  Ink is ``byte < threshold``, the rule of ``gather_u8``'s binarize and of ``d_score_u8``.

All three take a contiguous uint8 device tensor (N, H, W) or (N, 1, H, W) with 1 <= H <= 128 and W a multiple of 4 in
4..128, run one kernel on the current stream and never synchronise the host.  Arguments are validated before the library is
touched; there is no CPU path.  Everything is integer arithmetic: equal input gives bit-equal output."""
from typing import Optional

import torch

from . import _call, _lib
from ._call import as_int, ptr

# columns of component_stats (SIGGAN_CC_*)
INK, COMPONENTS, LARGEST, SMALL_COMPONENTS, SMALL_INK, X0, Y0, X1, Y1 = range(9)
STAT_NAMES = ("ink", "components", "largest", "small_components", "small_ink", "x0", "y0", "x1", "y1")


def default_min_area(height: int, width: int) -> int:
    """max(2, round(0.001 * height * width)) PIXELS: 4 at 64x64, 16 at 128x128.  The ratio is the reference's
    MIN_CONTOUR_AREA_RATIO (preprocess_signatures.py), but this counts the pixels of a component where the reference measures
    OpenCV's contour polygon area, so it is NOT the reference's number: a one-pixel-wide stroke has polygon area 0 and any
    pixel count."""
    return max(2, int(round(0.001 * int(height) * int(width))))


def check_arguments(u8, threshold, connectivity, min_area, fill=255):
    """The refusals that need no device, in a fixed order: type, dtype, rank, sizes, parameters, device, layout.
    Returns (n, h, w, threshold, connectivity, min_area, fill) with min_area resolved."""
    n, h, w = _call.check_u8_images(u8, "images", 1, 4, _lib.CC_MAX_SIZE, True)
    threshold, connectivity, fill = as_int(threshold, "threshold"), as_int(connectivity, "connectivity"), as_int(fill, "fill")
    min_area = default_min_area(h, w) if min_area is None else as_int(min_area, "min_area")
    if not 1 <= threshold <= 255:
        raise ValueError(f"threshold = {threshold} outside [1, 255]")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if min_area < 1:
        raise ValueError(f"min_area = {min_area} < 1")
    if not threshold <= fill <= 255:
        raise ValueError(f"fill = {fill} outside [threshold = {threshold}, 255]: a cleaned pixel must not be ink")
    _call.check_resident(u8, "images")
    return n, h, w, threshold, connectivity, min_area, fill


def _run(u8, n, h, w, threshold, connectivity, min_area, fill, stats=None, root=None, clean=None):
    if n == 0:
        return
    _lib.check(_lib.load().siggan_components_u8(_call.device_of(u8).index, ptr(u8), n, h, w, threshold, connectivity, min_area, fill,
                                                ptr(stats), ptr(root), ptr(clean), _call.stream(u8.device)))


def component_stats(u8: torch.Tensor, threshold: int = 128, connectivity: int = 8, min_area: Optional[int] = None) -> torch.Tensor:
    """int32 (N, 9) on the device: ink, components, largest, small_components, small_ink, x0, y0, x1, y1 (STAT_NAMES).
    ``min_area`` None: ``default_min_area(H, W)``.  The box is -1 where no component reaches min_area."""
    n, h, w, threshold, connectivity, min_area, fill = check_arguments(u8, threshold, connectivity, min_area)
    stats = torch.empty((n, 9), dtype=torch.int32, device=u8.device)
    _run(u8, n, h, w, threshold, connectivity, min_area, fill, stats=stats)
    return stats


def component_roots(u8: torch.Tensor, threshold: int = 128, connectivity: int = 8) -> torch.Tensor:
    """int32, the shape of ``u8``: -1 for background, else the smallest linear index y * W + x of the pixel's component."""
    n, h, w, threshold, connectivity, min_area, fill = check_arguments(u8, threshold, connectivity, 1)
    root = torch.empty(u8.shape, dtype=torch.int32, device=u8.device)
    _run(u8, n, h, w, threshold, connectivity, min_area, fill, root=root)
    return root


def despeckle_u8(u8: torch.Tensor, threshold: int = 128, connectivity: int = 8, min_area: Optional[int] = None, fill: int = 255,
                 out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8, the shape of ``u8``: every pixel of a component with fewer than ``min_area`` pixels becomes ``fill``, every other
    byte is the input's.  ``out`` may be ``u8`` itself (in place) or a contiguous uint8 tensor of the same element count that
    does not overlap it; ``stats``, a contiguous int32 (N, 9) device tensor, receives component_stats' counters of the INPUT
    from the same launch (small_components / small_ink are what the cleaning removes)."""
    n, h, w, threshold, connectivity, min_area, fill = check_arguments(u8, threshold, connectivity, min_area, fill)
    out = _call.check_out_u8(out, u8)
    _call.check_stats(stats, n, 9, u8.device)
    _run(u8, n, h, w, threshold, connectivity, min_area, fill, stats=stats, clean=out)
    return out
