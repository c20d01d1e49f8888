"""Pillow's antialiased bilinear resize on the device (include/siggan_resize.h, csrc/resize.hip).

The reference joins its two halves through files: the GAN writes 128x128 PNGs and the verifier's
``transforms.Resize((64, 64))`` shrinks them with ``Image.resize(..., Image.BILINEAR)`` before the network sees them.
``resize_u8`` is that step for uint8 images that never left the device (``Engine.g_generate_u8``), byte for byte;
``resize_f32`` is the same linear map on fp32 images without the byte roundings and ``resize_f32_adjoint`` its exact
transpose, so a gradient can cross the resize (``SiameseNetwork.input_grad_resized``).

All three take contiguous device tensors (N, H, W) or (N, 1, H, W), return the same rank (or fill ``out``, a caller-owned
contiguous tensor of the result's dtype and element count, and return it), run on the current stream and
never synchronise the host -- except that the first call with a new (in, out) axis pair on a device builds and uploads
that pair's coefficient table.  Arguments are validated before the library is touched; there is no CPU path.
``coefficient_table`` hands out the host-side table (no GPU needed)."""
import ctypes as C
from typing import Dict, Optional, Tuple, Union

import numpy as np
import torch

from . import _call, _lib

Size = Union[int, Tuple[int, int]]
_CONTEXTS: Dict[int, "_ResizeContext"] = {}


class _ResizeContext:
    """One siggan_resize handle per device: the cached coefficient tables."""

    def __init__(self, index: int):
        self.lib = _lib.load()
        h = C.c_void_p()
        _lib.check(self.lib.siggan_resize_create(index, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.siggan_resize_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # interpreter shutdown
            pass


def _context(src: torch.Tensor) -> _ResizeContext:
    index = _call.device_of(src).index
    ctx = _CONTEXTS.get(index)
    if ctx is None:
        ctx = _CONTEXTS[index] = _ResizeContext(index)
    return ctx


def _pair(size: Size, what: str, limit: int) -> Tuple[int, int]:
    if isinstance(size, (int, np.integer)) and not isinstance(size, bool):
        size = (size, size)
    if (not isinstance(size, (tuple, list)) or len(size) != 2
            or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in size)):
        raise ValueError(f"{what} must be an integer or a pair (height, width) of integers, got {size!r}")
    h, w = int(size[0]), int(size[1])
    if not (1 <= h <= limit and 1 <= w <= limit):
        raise ValueError(f"{what} = {h} x {w} outside [1, {limit}]")
    return h, w


def check_images(images, dtype: torch.dtype, what: str, limit: int) -> Tuple[int, int, int]:
    """The refusals that need no device, in a fixed order: type, dtype, rank, sizes, device, layout.  Returns (n, h, w)."""
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{what} must be a tensor, got {type(images).__name__}")
    if images.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {images.dtype}")
    if not (images.dim() == 3 or (images.dim() == 4 and images.shape[1] == 1)):
        raise ValueError(f"{what} must be (N, H, W) or (N, 1, H, W), got {tuple(images.shape)}")
    n, h, w = images.shape[0], images.shape[-2], images.shape[-1]
    if not (1 <= h <= limit and 1 <= w <= limit):
        raise ValueError(f"{what} is {h} x {w}: sizes outside [1, {limit}]")
    _call.check_resident(images, what)
    return n, h, w


def _run(name: str, src: torch.Tensor, n: int, hs: int, ws: int, hd: int, wd: int, out) -> torch.Tensor:
    if out is None:
        dst = torch.empty(src.shape[:-2] + (hd, wd), dtype=src.dtype, device=src.device)
    else:
        if (not isinstance(out, torch.Tensor) or out.dtype != src.dtype or out.device != src.device or not out.is_contiguous()
                or out.numel() != n * hd * wd):
            raise ValueError(f"out must be a contiguous {src.dtype} tensor of {n * hd * wd} elements on {src.device}")
        dst = out
    if n == 0:
        return dst
    ctx = _context(src)
    _lib.check(getattr(ctx.lib, name)(ctx._h, _call.ptr(src), n, hs, ws, _call.ptr(dst), hd, wd, _call.stream(src.device)))
    return dst


def resize_u8(images: torch.Tensor, size: Size = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 (N, H, W) -> uint8 (N, h, w): ``Image.fromarray(a).resize((w, h), Image.BILINEAR)`` of every image, byte for
    byte.  1 <= H, W <= 1024, 1 <= h, w <= 128."""
    hd, wd = _pair(size, "size", _lib.RESIZE_MAX_OUT)
    n, hs, ws = check_images(images, torch.uint8, "images", _lib.RESIZE_MAX_IN)
    return _run("siggan_resize_u8", images, n, hs, ws, hd, wd, out)


def resize_f32(images: torch.Tensor, size: Size = 64, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 (N, H, W) -> fp32 (N, h, w): y = R_h x R_w^T with Pillow's un-quantised weights rounded to fp32, horizontal pass
    first, fp32 intermediate, ascending tap order.  Sizes as resize_u8."""
    hd, wd = _pair(size, "size", _lib.RESIZE_MAX_OUT)
    n, hs, ws = check_images(images, torch.float32, "images", _lib.RESIZE_MAX_IN)
    return _run("siggan_resize_f32", images, n, hs, ws, hd, wd, out)


def resize_f32_adjoint(grad: torch.Tensor, in_hw: Size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 (N, h, w) gradient with respect to resize_f32's output -> the gradient (N, H, W) with respect to its input of
    size ``in_hw``: dx = R_h^T dy R_w, a gather in ascending output order (no atomics, bit-equal from run to run)."""
    hi, wi = _pair(in_hw, "in_hw", _lib.RESIZE_MAX_IN)
    n, ho, wo = check_images(grad, torch.float32, "grad", _lib.RESIZE_MAX_OUT)
    return _run("siggan_resize_f32_adjoint", grad, n, ho, wo, hi, wi, out)


def coefficient_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(bounds (out, 2) int32: window start and length; kk (out, ksize) int32: 22-bit weights; kf (out, ksize) float32)
    of one axis, from the library's host code (siggan_resize_table; needs no device)."""
    lib = _lib.load()
    ksize = lib.siggan_resize_ksize(int(n_in), int(n_out))
    if ksize < 0:
        _lib.check(ksize)
    bounds = np.zeros((n_out, 2), dtype=np.int32)
    kk = np.zeros((n_out, ksize), dtype=np.int32)
    kf = np.zeros((n_out, ksize), dtype=np.float32)
    _lib.check(lib.siggan_resize_table(int(n_in), int(n_out), C.c_void_p(bounds.ctypes.data), C.c_void_p(kk.ctypes.data),
                                       C.c_void_p(kf.ctypes.data)))
    return bounds, kk, kf
