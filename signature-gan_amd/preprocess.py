"""Scan preprocessing on the device (include/siggan_preprocess.h, csrc/preprocess.hip): from raw grayscale scans of any
size between 16 and 1024 pixels a side to the 64 x 64 or 128 x 128 byte images the rest of the package reads.

``pack_scans`` puts a list of (h, w) uint8 arrays back to back in one device pool with the geometry table and the workspace
the kernels need -- a ``ScanBatch``, reusable for any number of calls.  ``preprocess_scans`` runs the six stages (denoise,
validate, crop, area resize, centre, CLAHE; each but validate and resize can be switched off) in three kernels on the
current stream and never synchronises the host; it returns the images and an int32 (n, 13) counter table (STAT_NAMES).
``validity`` turns the WHITE counter into the reference's accept / reject decision on the host.

Every stage is exact integer arithmetic, restated in tests/preprocesscommon.py, and the kernels equal that restatement bit
for bit.  Which stages follow OpenCV's rule and which replace it is tabulated in DESIGN.md; agreement with an OpenCV build
is not measured.  Arguments are validated before the library is touched; there is no CPU path."""
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _call, _lib
from ._call import as_int, ptr

# columns of the counter table (SIGGAN_PP_*)
STATUS, WHITE, COMPONENTS, KEPT, CROP_X, CROP_Y, CROP_W, CROP_H, NEW_W, NEW_H, SHIFT_X, SHIFT_Y, M00 = range(13)
STAT_NAMES = ("status", "white", "components", "kept", "crop_x", "crop_y", "crop_w", "crop_h", "new_w", "new_h", "shift_x",
              "shift_y", "m00")
NO_BBOX, DEGENERATE, OVERFLOW = _lib.PP_NO_BBOX, _lib.PP_DEGENERATE, _lib.PP_OVERFLOW
# the reference's constants (preprocess_signatures.py)
MIN_CONTOUR_AREA_RATIO, MAX_NOISE_RATIO, MIN_INK_RATIO = 0.001, 0.95, 0.01


def default_min_pixels(height: int, width: int) -> int:
    """The smallest integer n with n > height * width * 0.001 as a Python float: a component is kept iff it has at least
    that many PIXELS.  The ratio is the reference's MIN_CONTOUR_AREA_RATIO, but the reference compares OpenCV's contour
    polygon area, which is 0 for a one-pixel line (components.default_min_area tells the same story)."""
    return math.floor(int(height) * int(width) * MIN_CONTOUR_AREA_RATIO) + 1


@dataclass
class ScanBatch:
    """A ragged batch on the device.  ``pool``: uint8 (total_pixels,), the scans back to back; ``geom`` / ``geom_host``:
    int64 (n, 4) {offset, height, width, min_pixels} on the device and on the host; ``workspace``: uint8, what the kernels
    scribble in (its content never matters)."""
    pool: torch.Tensor
    geom: torch.Tensor
    geom_host: torch.Tensor
    workspace: torch.Tensor

    @property
    def n(self) -> int:
        return self.geom_host.shape[0]

    @property
    def total_pixels(self) -> int:
        return self.pool.numel()

    def scan(self, i: int, pool: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Scan i as an (h, w) view of ``pool`` (default: the batch's own; e.g. a ``denoised=`` pool)."""
        off, h, w, _ = (int(v) for v in self.geom_host[i])
        return (self.pool if pool is None else pool)[off:off + h * w].view(h, w)


def check_scans(scans, min_pixels=None):
    """The refusals of pack_scans that need no device: type, dtype, rank, sizes, parameters.  Returns [(h, w, min_pixels)]."""
    if not isinstance(scans, (list, tuple)):
        raise ValueError(f"scans must be a list of (h, w) uint8 arrays, got {type(scans).__name__}")
    if not scans:
        raise ValueError("scans holds no scan")
    if len(scans) > _lib.PP_MAX_BATCH:
        raise ValueError(f"{len(scans)} scans exceed {_lib.PP_MAX_BATCH} in one batch")
    for i, a in enumerate(scans):
        if not isinstance(a, (np.ndarray, torch.Tensor)):
            raise ValueError(f"scan {i} must be a numpy array or a tensor, got {type(a).__name__}")
    for i, a in enumerate(scans):
        if a.dtype not in (np.uint8, torch.uint8):
            raise ValueError(f"scan {i} must be uint8, got {a.dtype}")
    for i, a in enumerate(scans):
        if a.ndim != 2:
            raise ValueError(f"scan {i} must be (h, w), got {tuple(a.shape)}")
    for i, a in enumerate(scans):
        h, w = a.shape
        if not _lib.PP_MIN_SIDE <= h <= _lib.PP_MAX_SIDE:
            raise ValueError(f"scan {i}: height = {h} outside [{_lib.PP_MIN_SIDE}, {_lib.PP_MAX_SIDE}]")
        if not _lib.PP_MIN_SIDE <= w <= _lib.PP_MAX_SIDE:
            raise ValueError(f"scan {i}: width = {w} outside [{_lib.PP_MIN_SIDE}, {_lib.PP_MAX_SIDE}]")
    if min_pixels is None:
        mp = [default_min_pixels(*a.shape) for a in scans]
    elif isinstance(min_pixels, (list, tuple, np.ndarray)):
        if len(min_pixels) != len(scans):
            raise ValueError(f"min_pixels holds {len(min_pixels)} values for {len(scans)} scans")
        mp = [as_int(v, "min_pixels") for v in min_pixels]
    else:
        mp = [as_int(min_pixels, "min_pixels")] * len(scans)
    for i, v in enumerate(mp):
        if v < 1:
            raise ValueError(f"scan {i}: min_pixels = {v} < 1")
    return [(int(a.shape[0]), int(a.shape[1]), v) for a, v in zip(scans, mp)]


def workspace_bytes(total_pixels: int, n: int) -> int:
    """siggan_preprocess_workspace: about 5.1 bytes per pixel and 17 KiB per scan."""
    return int(_lib.load().siggan_preprocess_workspace(int(total_pixels), int(n)))


def pack_scans(scans: Sequence, device="cuda", min_pixels=None) -> ScanBatch:
    """One host copy and one upload: the scans back to back in the order given, their geometry, a workspace.
    ``min_pixels``: None (``default_min_pixels`` per scan), one integer, or one per scan."""
    sizes = check_scans(scans, min_pixels)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"device must be {_call.ROCM_DEVICE}")
    geom = np.zeros((len(sizes), 4), dtype=np.int64)
    off = 0
    for i, (h, w, mp) in enumerate(sizes):
        geom[i] = (off, h, w, mp)
        off += h * w
    pool = np.empty(off, dtype=np.uint8)
    for a, g in zip(scans, geom):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        pool[g[0]:g[0] + g[1] * g[2]] = np.ascontiguousarray(a).reshape(-1)
    geom_host = torch.from_numpy(geom)
    return ScanBatch(torch.from_numpy(pool).to(device), geom_host.to(device), geom_host,
                     torch.empty(workspace_bytes(off, len(sizes)), dtype=torch.uint8, device=device))


def check_arguments(batch, size, margin, out, stats, denoised, canvas):
    """type, sizes, parameters, device, layout.  Returns (n, size, margin)."""
    if not isinstance(batch, ScanBatch):
        raise ValueError(f"batch must be a ScanBatch (pack_scans), got {type(batch).__name__}")
    size, margin = as_int(size, "size"), as_int(margin, "margin")
    if size not in (64, 128):
        raise ValueError(f"size must be 64 or 128, got {size}")
    if not 0 <= margin <= _lib.PP_MAX_MARGIN:
        raise ValueError(f"margin = {margin} outside [0, {_lib.PP_MAX_MARGIN}]")
    n, dev = batch.n, batch.pool.device
    if dev.type != "cuda":
        raise ValueError(f"batch must live on {_call.ROCM_DEVICE}")
    for name, t, shape in (("out", out, (n, size, size)), ("canvas", canvas, (n, size, size)), ("denoised", denoised, (batch.total_pixels,))):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous()
                              or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be a contiguous torch.uint8 tensor {shape} on {dev}")
    _call.check_stats(stats, n, _lib.PP_COUNT, dev)
    return n, size, margin


def preprocess_scans(batch: ScanBatch, size: int = 64, denoise: bool = True, crop: bool = True, center: bool = True,
                     equalize: bool = True, margin: int = 5, out: Optional[torch.Tensor] = None, stats: Optional[torch.Tensor] = None,
                     denoised: Optional[torch.Tensor] = None, canvas: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(uint8 (n, size, size), int32 (n, 13)) on the batch's device.  ``out`` / ``stats``: caller-owned tensors of those
    shapes to write into.  ``denoised``: a uint8 (total_pixels,) tensor that receives stage 1's result, laid out like the
    pool; ``canvas``: a uint8 (n, size, size) tensor that receives the image before the equalisation -- how each stage can
    be looked at alone.  A scan whose status has DEGENERATE set is all 255; OVERFLOW means a bug in the labelling."""
    n, size, margin = check_arguments(batch, size, margin, out, stats, denoised, canvas)
    dev = batch.pool.device
    out = torch.empty((n, size, size), dtype=torch.uint8, device=dev) if out is None else out
    stats = torch.empty((n, _lib.PP_COUNT), dtype=torch.int32, device=dev) if stats is None else stats
    opt = _lib.PreprocessOptions(size, int(bool(denoise)), int(bool(crop)), int(bool(center)), int(bool(equalize)), margin)
    _lib.check(_lib.load().siggan_preprocess_u8(_call.device_of(batch.pool).index, ptr(batch.pool), batch.total_pixels,
                                                ptr(batch.geom_host), ptr(batch.geom), n, opt, ptr(out), ptr(stats), ptr(denoised),
                                                ptr(canvas), ptr(batch.workspace), batch.workspace.numel(), _call.stream(dev)))
    return out, stats


def validity(stats, geom) -> np.ndarray:
    """bool (n,): stage 2's decision, with the reference's own expressions -- a scan is rejected iff more than
    MAX_NOISE_RATIO of its denoised pixels are white (> 127) or fewer than MIN_INK_RATIO are not.  ``stats``: the counter
    table (device tensor or array; a device tensor is copied to the host here); ``geom``: the (n, 4) geometry table."""
    s = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    g = geom.cpu().numpy() if isinstance(geom, torch.Tensor) else np.asarray(geom)
    ok = np.zeros(len(s), dtype=bool)
    for i in range(len(s)):
        total_pixels = int(g[i, 1]) * int(g[i, 2])
        white_pixels = int(s[i, WHITE])
        dark_pixels = total_pixels - white_pixels
        ok[i] = not (white_pixels / total_pixels > MAX_NOISE_RATIO or dark_pixels / total_pixels < MIN_INK_RATIO)
    return ok
