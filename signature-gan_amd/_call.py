"""The calling convention the wrappers of the context-free ops share: how a tensor becomes a pointer, which stream a call
runs on, and the refusals that need no device.

Plain functions.  None of them launches, copies or synchronises anything.  A refusal is a ValueError whose text names the
argument; where two ops word one refusal differently the wording is an argument, so every op keeps its own messages.  The
order inside a helper is fixed: type, dtype, rank, sizes -- and, as a call of its own (``check_resident``), device, layout,
because an op checks its own parameters between the two."""
import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

ROCM_DEVICE = "a ROCm device ('cuda:N'); there is no CPU path"


def ptr(t: Optional[torch.Tensor]) -> C.c_void_p:
    """The tensor's address; NULL for None."""
    return C.c_void_p(t.data_ptr() if t is not None else None)


def stream(device: torch.device) -> C.c_void_p:
    """torch's current stream on ``device``: every op enqueues there."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_of(t: torch.Tensor) -> torch.device:
    """The tensor's device with its index resolved (a bare 'cuda' is the current device)."""
    dev = t.device
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _name(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def as_int(value, what: str) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{what} must be an integer, got {value!r}")
    return int(value)


def check_u8_images(u8, what: str = "images", min_h: int = 1, min_w: int = 4, max_size: int = 128, allow_empty: bool = True,
                    kinds: str = "a tensor") -> Tuple[int, int, int]:
    """Byte images (N, H, W) or (N, 1, H, W), min_h <= H <= max_size, W a multiple of 4 in min_w..max_size: type, dtype,
    rank, sizes.  ``kinds``: what the type refusal says may be passed.  Returns (n, h, w)."""
    if not isinstance(u8, torch.Tensor):
        raise ValueError(f"{what} must be {kinds}, got {type(u8).__name__}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"{what} must be torch.uint8, got {u8.dtype}")
    if not (u8.dim() == 3 or (u8.dim() == 4 and u8.shape[1] == 1)):
        raise ValueError(f"{what} must be (N, H, W) or (N, 1, H, W), got {tuple(u8.shape)}")
    n, h, w = u8.shape[0], u8.shape[-2], u8.shape[-1]
    if n < 1 and not allow_empty:
        raise ValueError(f"{what} holds no image")
    if not min_h <= h <= max_size:
        raise ValueError(f"height = {h} outside [{min_h}, {max_size}]")
    if not min_w <= w <= max_size or w % 4:
        raise ValueError(f"width = {w} must be a multiple of 4 in [{min_w}, {max_size}]")
    return n, h, w


def check_resident(t: torch.Tensor, what: str = "images") -> None:
    """Device, then layout."""
    if t.device.type != "cuda":
        raise ValueError(f"{what} must live on {ROCM_DEVICE}")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def check_rows(name: str, t, dtype: torch.dtype, shape_text: str, shape: Sequence[Optional[int]] = (None, None), min_rows: int = 0,
               device: Optional[torch.device] = None, where: str = ROCM_DEVICE, contiguous: bool = True) -> None:
    """A ``dtype`` tensor whose sizes match ``shape`` (None: any) with at least ``min_rows`` rows: residence -- on ``device``,
    or on any ROCm device when that is None; ``where`` is how the refusal names the place --, then dtype and sizes
    (``shape_text`` is how the refusal names them), then layout."""
    if not isinstance(t, torch.Tensor) or (t.device.type != "cuda" if device is None else t.device != device):
        raise ValueError(f"{name} must be a tensor on {where}")
    if (t.dtype != dtype or t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape))
            or t.shape[0] < min_rows):
        raise ValueError(f"{name} must be {_name(dtype)} {shape_text}, got {t.dtype} {tuple(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def check_vector(name: str, t, dtype: torch.dtype, n: int, dev: torch.device) -> None:
    if (not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != dtype or tuple(t.shape) != (n,)
            or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {_name(dtype)} ({n},) tensor on {dev}")


def check_out_u8(out, u8: torch.Tensor) -> torch.Tensor:
    """The byte output of an op that may work in place: None -> a new tensor like ``u8``; else ``u8`` itself or a tensor of
    its element count that does not overlap it."""
    if out is None:
        return torch.empty_like(u8)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != u8.device or not out.is_contiguous()
            or out.numel() != u8.numel()):
        raise ValueError(f"out must be a contiguous torch.uint8 tensor of {u8.numel()} elements on {u8.device}")
    if out.data_ptr() != u8.data_ptr() and (out.data_ptr() < u8.data_ptr() + u8.numel() and u8.data_ptr() < out.data_ptr() + out.numel()):
        raise ValueError("out overlaps the input without being the input")
    return out


def check_stats(stats, n: int, count: int, dev: torch.device) -> None:
    """An optional caller-owned int32 (n, count) counter tensor."""
    if stats is not None and (not isinstance(stats, torch.Tensor) or stats.dtype != torch.int32 or stats.device != dev
                              or not stats.is_contiguous() or tuple(stats.shape) != (n, count)):
        raise ValueError(f"stats must be a contiguous torch.int32 tensor ({n}, {count}) on {dev}")
