"""The signature duplicator on the device: smooth random warps of byte images (include/siggan_warp.h, csrc/warp.hip).

One real signature in, many plausible same-writer variants out: a free-form cubic B-spline deformation -- a coarse grid of
random control displacements, interpolated smoothly -- on top of a small random affine (rotation, slant, scale, shift about
the image centre), resampled bilinearly.  Hand-to-hand variation is mostly local stretching and shifting, which is what the
control grid produces and what no rigid augmentation of the package does.  The header states the arithmetic in full; it is
integer arithmetic throughout, restated in tests/warpcommon.py, and the kernel equals that restatement bit for bit.

``WarpSpec`` says how strong the warp is; ``warp_u8`` applies it to contiguous uint8 device tensors (N, H, W) or
(N, 1, H, W), 1 <= H <= 128, W a multiple of 4 in 4..128, on the current stream without synchronising the host;
``duplicate_u8`` makes ``copies`` variants of every image.  Every output image has a 64-bit draw id: with the seed it
decides the control displacements and the affine draws, so an image's result does not depend on its place in the batch.
The control amplitude is limited to 0.4 cells per axis, the known sufficient bound for a deformation that does not fold
(Choi & Lee 2000); ``ctrl=`` hands in a control grid of the caller's own, whose folds are the caller's business.

Arguments are validated before the library is touched; there is no CPU path.  ``draw_affine``, ``control_grid_shape``,
``max_amplitude`` and ``WarpSpec.check`` need no device."""
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _call, _lib
from ._call import as_int, ptr

CELLS = _lib.WARP_CELLS
IDENTITY = (65536, 0, 0, 0, 65536, 0)
AFFINE_DRAWS = ("rotate_deg", "slant", "scale", "shift_x", "shift_y")


def max_amplitude(cell: int) -> int:
    """floor(0.4 * cell * 256): the largest control amplitude in Q8 (1/256 pixel) -- 819, 1638, 3276."""
    cell = as_int(cell, "cell")
    if cell not in CELLS:
        raise ValueError(f"cell must be one of {CELLS}, got {cell}")
    return cell * 512 // 5


def control_grid_shape(h: int, w: int, cell: int) -> Tuple[int, int]:
    """(gy, gx) = (ceil(h / cell) + 3, ceil(w / cell) + 3): the control points of an (h, w) image."""
    h, w, cell = as_int(h, "h"), as_int(w, "w"), as_int(cell, "cell")
    if cell not in CELLS:
        raise ValueError(f"cell must be one of {CELLS}, got {cell}")
    if h < 1 or w < 1:
        raise ValueError(f"h and w must be positive, got {h} and {w}")
    return -(-h // cell) + 3, -(-w // cell) + 3


def _real(value, what: str) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value):
        raise ValueError(f"{what} must be a finite number, got {value!r}")
    return float(value)


@dataclass(frozen=True)
class WarpSpec:
    """How strong a warp is.  ``cell``: pixels between control points (8, 16, 32; a larger cell is a smoother warp);
    ``amplitude``: (ax, ay), the largest control displacement per axis in pixels, one number for both, at most 0.4 cells;
    per image and uniformly drawn: a rotation within +-``rotate_deg`` degrees, a horizontal slant within +-``slant`` (pixels
    of x per pixel of y), a scale within 1 +- ``scale`` and a shift within +-``shift_px`` pixels per axis, all about the
    image centre; ``fill``: the byte read outside the source image (255 is paper)."""
    cell: int = 16
    amplitude: Union[float, Tuple[float, float]] = (2.0, 2.0)
    rotate_deg: float = 0.0
    slant: float = 0.0
    scale: float = 0.0
    shift_px: float = 0.0
    fill: int = 255

    def amplitude_q8(self) -> Tuple[int, int]:
        """(amp_x, amp_y) in Q8, rounded to nearest."""
        a = self.amplitude if isinstance(self.amplitude, (tuple, list)) else (self.amplitude, self.amplitude)
        return tuple(int(math.floor(float(v) * 256.0 + 0.5)) for v in a)

    def has_affine(self) -> bool:
        return any(float(v) != 0.0 for v in (self.rotate_deg, self.slant, self.scale, self.shift_px))

    def check(self) -> "WarpSpec":
        """The refusals, none of which needs a device: cell, amplitude, the affine ranges, fill.  Returns self."""
        cell = as_int(self.cell, "cell")
        if cell not in CELLS:
            raise ValueError(f"cell must be one of {CELLS}, got {cell}")
        a = self.amplitude if isinstance(self.amplitude, (tuple, list)) else (self.amplitude, self.amplitude)
        if len(a) != 2:
            raise ValueError(f"amplitude must be one number or (ax, ay), got {self.amplitude!r}")
        for v, axis in zip(a, "xy"):
            _real(v, f"amplitude {axis}")
        for q, axis in zip(self.amplitude_q8(), "xy"):
            if not 0 <= q <= max_amplitude(cell):
                raise ValueError(f"amplitude {axis} = {q} / 256 px outside [0, {max_amplitude(cell)} / 256] (0.4 cells of {cell} px)")
        for name in ("rotate_deg", "slant", "scale", "shift_px"):
            if _real(getattr(self, name), name) < 0:
                raise ValueError(f"{name} = {getattr(self, name)} < 0")
        if self.rotate_deg > 45:
            raise ValueError(f"rotate_deg = {self.rotate_deg} outside [0, 45]")
        if self.slant > 1:
            raise ValueError(f"slant = {self.slant} outside [0, 1]")
        if self.scale > 0.5:
            raise ValueError(f"scale = {self.scale} outside [0, 0.5]")
        if self.shift_px > _lib.WARP_MAX_SIZE:
            raise ValueError(f"shift_px = {self.shift_px} outside [0, {_lib.WARP_MAX_SIZE}]")
        fill = as_int(self.fill, "fill")
        if not 0 <= fill <= 255:
            raise ValueError(f"fill = {fill} outside [0, 255]")
        return self


def check_seed(seed, what: str = "seed") -> int:
    seed = as_int(seed, what)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{what} = {seed} outside [0, 2^64)")
    return seed


def check_draw_ids(draw_ids, n: int) -> np.ndarray:
    """None: 0 .. n - 1.  Else n integers in [0, 2^64), as uint64."""
    if draw_ids is None:
        return np.arange(n, dtype=np.uint64)
    if isinstance(draw_ids, np.ndarray) and draw_ids.ndim == 1 and draw_ids.dtype.kind in "iu":       # no Python loop over a large batch
        if draw_ids.dtype.kind == "i" and (draw_ids < 0).any():
            raise ValueError(f"draw id = {int(draw_ids[draw_ids < 0][0])} outside [0, 2^64)")
        if len(draw_ids) != n:
            raise ValueError(f"draw_ids holds {len(draw_ids)} values for {n} images")
        return draw_ids.astype(np.uint64)
    ids = [check_seed(v, "draw id") for v in (draw_ids.tolist() if isinstance(draw_ids, (np.ndarray, torch.Tensor)) else list(draw_ids))]
    if len(ids) != n:
        raise ValueError(f"draw_ids holds {len(ids)} values for {n} images")
    return np.array(ids, dtype=np.uint64)


def affine_fixed(rotate_deg, slant, scale, shift_x, shift_y, h: int, w: int) -> np.ndarray:
    """The 16.16 base map {a0 .. a5} of include/siggan_warp.h for arrays of draws, int32 (n, 6): output pixel (x, y) reads the
    source at A^-1 (x - cx, y - cy) + (cx, cy) - shift with A = scale * R(rotate) * [[1, slant], [0, 1]] and (cx, cy) =
    ((w - 1) / 2, (h - 1) / 2), pixel indices being pixel centres; each number is floor(v * 65536 + 0.5).  All-zero draws at
    scale 1 give the identity exactly."""
    rot = np.radians(np.asarray(rotate_deg, np.float64).reshape(-1))
    k, s = np.asarray(slant, np.float64).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
    tx, ty = np.asarray(shift_x, np.float64).reshape(-1), np.asarray(shift_y, np.float64).reshape(-1)
    cos, sin = np.cos(rot), np.sin(rot)
    # A = s [[cos, -sin], [sin, cos]] [[1, k], [0, 1]] = s [[cos, k cos - sin], [sin, k sin + cos]], det A = s^2
    m00, m01, m10, m11 = (k * sin + cos) / s, -(k * cos - sin) / s, -sin / s, cos / s
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    m02 = cx - m00 * cx - m01 * cy - tx
    m12 = cy - m10 * cx - m11 * cy - ty
    return np.stack([np.floor(v * 65536.0 + 0.5) for v in (m00, m01, m02, m10, m11, m12)], 1).astype(np.int64).astype(np.int32)


def draw_affine(spec: WarpSpec, n: int, seed: int, size: Tuple[int, int], draw_ids=None) -> Tuple[np.ndarray, Dict[str, np.ndarray]]:
    """(int32 (n, 6), the draws): image i's five uniform draws -- rotation, slant, scale, shift x, shift y, in that order --
    come from ``np.random.default_rng((seed, draw id))``, so they depend on the seed and the image's draw id alone
    (``draw_ids`` None: 0 .. n - 1); ``size`` = (h, w) places the centre.  A spec without affine ranges draws nothing and
    gives the identity."""
    spec.check()
    n, seed = as_int(n, "n"), check_seed(seed)
    h, w = (as_int(v, "size") for v in size)
    ids = check_draw_ids(draw_ids, n)
    d = np.zeros((n, 5), np.float64)
    d[:, 2] = 1.0
    if spec.has_affine():
        lo = np.array([-spec.rotate_deg, -spec.slant, 1.0 - spec.scale, -spec.shift_px, -spec.shift_px], np.float64)
        hi = np.array([spec.rotate_deg, spec.slant, 1.0 + spec.scale, spec.shift_px, spec.shift_px], np.float64)
        for i in range(n):
            d[i] = np.random.default_rng((seed, int(ids[i]))).uniform(lo, hi)
    draws = {name: d[:, k].copy() for k, name in enumerate(AFFINE_DRAWS)}
    return affine_fixed(*(draws[name] for name in AFFINE_DRAWS), h, w), draws


def param_rows(draw_ids: np.ndarray, amp_q8: Tuple[int, int], affine: np.ndarray) -> np.ndarray:
    """int32 (n, 12): {draw id low, high, amp_x, amp_y, a0 .. a5, 0, 0} -- the kernel's parameter rows."""
    n = len(draw_ids)
    rows = np.zeros((n, _lib.WARP_PARAMS), np.int32)
    ids = np.asarray(draw_ids, np.uint64)
    rows[:, 0] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    rows[:, 1] = (ids >> np.uint64(32)).astype(np.uint32).view(np.int32)
    rows[:, 2], rows[:, 3] = amp_q8
    rows[:, 4:10] = affine
    return rows


def check_arguments(u8, spec, seed, draw_ids, index, ctrl, out, affine):
    """type, dtype, rank, sizes; the spec; seed, index, draw ids, affine; then device and layout; then ctrl and out.
    Returns (n_src, h, w, n, seed, draw ids, index or None, affine or None)."""
    n_src, h, w = _call.check_u8_images(u8, "images", 1, 4, _lib.WARP_MAX_SIZE, False)
    if not isinstance(spec, WarpSpec):
        raise ValueError(f"spec must be a WarpSpec, got {type(spec).__name__}")
    spec.check()
    seed = check_seed(seed)
    if index is not None:
        if isinstance(index, torch.Tensor):
            index = index.cpu().numpy()
        index = np.asarray(index)
        if index.ndim != 1 or index.dtype.kind not in "iu" or not len(index):
            raise ValueError(f"index must be a non-empty 1-D integer array, got {index.dtype} {index.shape}")
        index = np.clip(index.astype(np.int64), -(1 << 31), (1 << 31) - 1).astype(np.int32)      # the kernel clamps into the images
    n = n_src if index is None else len(index)
    if n > _lib.WARP_MAX_N:
        raise ValueError(f"{n} output images exceed {_lib.WARP_MAX_N} in one call")
    ids = check_draw_ids(draw_ids, n)
    if affine is not None:
        affine = np.asarray(affine)
        if affine.shape != (n, 6) or affine.dtype.kind not in "iu" or np.abs(affine.astype(np.int64)).max() >= 1 << 31:
            raise ValueError(f"affine must be ({n}, 6) integers that fit int32, got {affine.dtype} {affine.shape}")
        affine = affine.astype(np.int32)
    _call.check_resident(u8, "images")
    dev = _call.device_of(u8)
    gy, gx = control_grid_shape(h, w, spec.cell)
    if ctrl is not None:
        _call.check_rows("ctrl", ctrl, torch.int16, f"({n}, 2, {gy}, {gx})", (n, 2, gy, gx), device=dev, where=str(dev))
    if out is not None:
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous()
                or tuple(out.shape) != (n, h, w)):
            raise ValueError(f"out must be a contiguous torch.uint8 tensor ({n}, {h}, {w}) on {dev}")
        if out.data_ptr() < u8.data_ptr() + u8.numel() and u8.data_ptr() < out.data_ptr() + out.numel():
            raise ValueError("out overlaps the images")
    return n_src, h, w, n, seed, ids, index, affine


def warp_u8(u8: torch.Tensor, spec: WarpSpec, seed: int, draw_ids: Optional[Sequence[int]] = None, index=None,
            ctrl: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, return_field: bool = False, affine=None):
    """uint8 (n, H, W) on the images' device: output i is the warp of image ``index[i]`` (None: i; an index outside the
    images is clamped into them) with draw id ``draw_ids[i]`` (None: i).  ``affine``: int (n, 6) 16.16 base maps that
    replace ``draw_affine(spec, n, seed, (H, W), draw_ids)``; ``ctrl``: int16 (n, 2, gy, gx) control displacements in Q8 on
    the device that replace the draws (clamped into +-8192; x plane first); ``out``: a caller-owned tensor that does not
    overlap the images; ``return_field``: also return the int32 (n, 2, H, W) Q8 displacement before the affine."""
    n_src, h, w, n, seed, ids, index, affine = check_arguments(u8, spec, seed, draw_ids, index, ctrl, out, affine)
    dev = _call.device_of(u8)
    if affine is None:
        affine = draw_affine(spec, n, seed, (h, w), ids)[0]
    rows = torch.from_numpy(param_rows(ids, spec.amplitude_q8(), affine)).to(dev)
    index_dev = torch.from_numpy(index).to(dev) if index is not None else None
    out = torch.empty((n, h, w), dtype=torch.uint8, device=dev) if out is None else out
    field = torch.empty((n, 2, h, w), dtype=torch.int32, device=dev) if return_field else None
    _lib.check(_lib.load().siggan_warp_u8(dev.index, ptr(u8), n_src, ptr(index_dev), ptr(rows), ptr(ctrl), ptr(out), ptr(field), n, h, w,
                                          int(spec.cell), int(spec.fill), seed, _call.stream(dev)))
    return (out, field) if return_field else out


def check_copies(copies) -> int:
    copies = as_int(copies, "copies")
    if copies < 1:
        raise ValueError(f"copies = {copies} < 1")
    return copies


def duplicate_u8(u8: torch.Tensor, copies: int, spec: WarpSpec, seed: int, first_id: int = 0, return_field: bool = False):
    """uint8 (N * copies, H, W): copy k of image i lands at row i * copies + k with draw id first_id + i * copies + k."""
    n_src, _, _ = _call.check_u8_images(u8, "images", 1, 4, _lib.WARP_MAX_SIZE, False)
    copies, first_id = check_copies(copies), check_seed(first_id, "first_id")
    n = n_src * copies
    if first_id + n > 1 << 64:
        raise ValueError(f"first_id = {first_id}: the draw ids of {n} copies leave [0, 2^64)")
    return warp_u8(u8, spec, seed, draw_ids=[first_id + r for r in range(n)], index=np.repeat(np.arange(n_src, dtype=np.int32), copies),
                   return_field=return_field)
