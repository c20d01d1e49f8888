"""Stroke geometry of byte images on the device (include/siggan_strokes.h, csrc/strokes.hip).

Neither a count of ink pixels nor a count of ink components says how thick a stroke is.  ``stroke_stats`` gives, per image,
the ink, the length of the skeleton (the centre line by Guo-Hall parallel thinning), its line ends and junction pixels, the
largest squared distance from ink to paper and a histogram of local pen widths along the skeleton; ``distance_map`` the exact
squared Euclidean distance of every ink pixel to the nearest background pixel; ``skeleton_u8`` the skeleton as 0/1 bytes;
``restroke_u8`` the skeleton drawn again with a disc of squared radius ``radius2`` -- the pen-width redraw.  Ink is
``byte < threshold``, the rule of ``components``; pixels outside the image are background.

A skeleton pixel with (k - 1)^2 < D2 <= k^2 is counted in width bin k and stands for a local pen width of 2k - 1.  An
axis-aligned bar of width W lands in bin ceil(W / 2): even widths read one pixel low.  This is documented, not corrected.

All four take a contiguous uint8 device tensor (N, H, W) or (N, 1, H, W) with 1 <= H <= 128 and W a multiple of 4 in
4..128, run one kernel on the current stream and never synchronise the host.  Arguments are validated before the library is
touched; there is no CPU path.  Everything is integer arithmetic: equal input gives bit-equal output."""
from typing import Optional

import torch

from . import _call, _lib
from ._call import as_int, ptr

# columns of stroke_stats (SIGGAN_SK_*)
INK, SKELETON, ENDPOINTS, JUNCTION_PIXELS, PASSES, D2_MAX, D2_SKEL_SUM, WIDTH_HIST = range(8)
WIDTH_BINS = _lib.SK_WIDTH_BINS
COUNT = WIDTH_HIST + WIDTH_BINS
STAT_NAMES = ("ink", "skeleton", "endpoints", "junction_pixels", "passes", "d2_max", "d2_skel_sum") + tuple(
    f"width_hist_{k}" for k in range(1, WIDTH_BINS + 1))
MAX_PEN_WIDTH = 9


def radius2_for_pen_width(w: int) -> int:
    """The squared disc radius that redraws a centre line at pen width ``w`` in 1..9: (w - 1)^2 // 4, that is
    0, 0, 1, 2, 4, 6, 9, 12, 16.  (Widths 1 and 2 both give the skeleton itself: it is one pixel wide.)"""
    w = as_int(w, "pen width")
    if not 1 <= w <= MAX_PEN_WIDTH:
        raise ValueError(f"pen width = {w} outside [1, {MAX_PEN_WIDTH}]")
    return (w - 1) ** 2 // 4


def check_arguments(u8, threshold, radius2=0, ink=0, fill=255):
    """The refusals that need no device, in a fixed order: type, dtype, rank, sizes, parameters, device, layout.
    Returns (n, h, w, threshold, radius2, ink, fill)."""
    n, h, w = _call.check_u8_images(u8, "images", 1, 4, _lib.SK_MAX_SIZE, True)
    threshold, radius2, ink, fill = as_int(threshold, "threshold"), as_int(radius2, "radius2"), as_int(ink, "ink"), as_int(fill, "fill")
    if not 1 <= threshold <= 255:
        raise ValueError(f"threshold = {threshold} outside [1, 255]")
    if not 0 <= radius2 <= _lib.SK_MAX_RADIUS2:
        raise ValueError(f"radius2 = {radius2} outside [0, {_lib.SK_MAX_RADIUS2}]")
    if not 0 <= ink < threshold:
        raise ValueError(f"ink = {ink} outside [0, threshold - 1 = {threshold - 1}]: a redrawn stroke must be ink")
    if not threshold <= fill <= 255:
        raise ValueError(f"fill = {fill} outside [threshold = {threshold}, 255]: the paper must not be ink")
    _call.check_resident(u8, "images")
    return n, h, w, threshold, radius2, ink, fill


def _run(u8, n, h, w, threshold, radius2=0, ink=0, fill=255, stats=None, d2=None, skel=None, redraw=None):
    if n == 0:
        return
    _lib.check(_lib.load().siggan_strokes_u8(_call.device_of(u8).index, ptr(u8), n, h, w, threshold, radius2, ink, fill, ptr(stats),
                                             ptr(d2), ptr(skel), ptr(redraw), _call.stream(u8.device)))


def stroke_stats(u8: torch.Tensor, threshold: int = 128) -> torch.Tensor:
    """int32 (N, 23) on the device: ink, skeleton, endpoints, junction_pixels, passes, d2_max, d2_skel_sum and the sixteen
    width bins (STAT_NAMES).  ``passes`` is -1 where the kernel's safety bound was reached, which no input should do."""
    n, h, w, threshold, *_ = check_arguments(u8, threshold)
    stats = torch.empty((n, COUNT), dtype=torch.int32, device=u8.device)
    _run(u8, n, h, w, threshold, stats=stats)
    return stats


def distance_map(u8: torch.Tensor, threshold: int = 128) -> torch.Tensor:
    """int16, the shape of ``u8``: the squared Euclidean distance of every ink pixel to the nearest background pixel (the
    pixels outside the image are background), 0 on background, at most 4096."""
    n, h, w, threshold, *_ = check_arguments(u8, threshold)
    d2 = torch.empty(u8.shape, dtype=torch.int16, device=u8.device)
    _run(u8, n, h, w, threshold, d2=d2)
    return d2


def skeleton_u8(u8: torch.Tensor, threshold: int = 128) -> torch.Tensor:
    """uint8, the shape of ``u8``: 1 on the skeleton, 0 elsewhere."""
    n, h, w, threshold, *_ = check_arguments(u8, threshold)
    skel = torch.empty_like(u8)
    _run(u8, n, h, w, threshold, skel=skel)
    return skel


def restroke_u8(u8: torch.Tensor, radius2: int, threshold: int = 128, ink: int = 0, fill: int = 255,
                out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8, the shape of ``u8``: ``ink`` wherever a skeleton pixel lies within squared distance ``radius2`` (0..36), ``fill``
    elsewhere; ``radius2`` = 0 draws the skeleton itself, ``radius2_for_pen_width(w)`` a pen of width ``w``.  ``out`` may be
    ``u8`` itself (in place) or a contiguous uint8 tensor of the same element count that does not overlap it; ``stats``, a
    contiguous int32 (N, 23) device tensor, receives stroke_stats' counters of the INPUT from the same launch."""
    n, h, w, threshold, radius2, ink, fill = check_arguments(u8, threshold, radius2, ink, fill)
    out = _call.check_out_u8(out, u8)
    _call.check_stats(stats, n, COUNT, u8.device)
    _run(u8, n, h, w, threshold, radius2, ink, fill, stats=stats, redraw=out)
    return out
