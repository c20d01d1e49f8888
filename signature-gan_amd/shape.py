"""Shape attributes of signature images on the device (include/siggan_shape.h, csrc/shape.hip): the ink moments up to second
order, a quadratic objective on them and its gradient with respect to the pixels.

Pixel (row r, column c) of an s x s image (s = 64 or 128) has the coordinates u = (c + 0.5) / s - 0.5, v = (r + 0.5) / s - 0.5;
v grows DOWNWARDS.  The ink of an fp32 pixel x is a = (1 - x) / 2, in fp64, not clamped; S0 = sum a, and an image with S0 <= 0
is empty.  The eight features (``FEATURES``): mass = S0 / s^2; cx, cy the ink's centre; sxx, syy, sxy its central second
moments (divided by S0); slant = sxy / syy (0 when syy <= 1e-12); spread = sxx + syy.  An empty image has features 1..7 = 0.

Slant is the shear coefficient: shearing an image by x' = x + k y adds k to it.  Because v points down, a signature that leans
to the RIGHT ("/") has a NEGATIVE slant.

``shape_features`` / ``shape_grad`` run one kernel on the current stream and never synchronise the host; the objective of
``shape_grad`` is 0.5 * sum_k w_k (f_k - t_k)^2 per image and dx its gradient with respect to the pixels -- the image-space
seed Engine.g_latent_objective_grad(image_grad=...) carries to the latent vector (utils.inference.edit_latents).  A feature
with weight 0 is skipped and its target is not looked at; on an empty image only the mass term contributes, and the slant
term contributes nothing when syy <= 1e-12.  ``shape_sums_u8`` gives the six exact integer sums of byte images (ink
255 - b, coordinates p = 2c + 1 - s, q = 2r + 1 - s) and ``features_from_sums`` turns them into the eight features on the
host, for ink (255 - b) / 255.  ``reference_features`` / ``reference_grad`` restate the definitions in numpy fp64; they need
no device.  Arguments are validated before the library is touched; there is no CPU path for the device calls."""
from typing import Optional, Tuple

import numpy as np
import torch

from . import _call, _lib
from ._call import device_of, ptr, stream

FEATURES = ("mass", "cx", "cy", "sxx", "syy", "sxy", "slant", "spread")
MASS, CX, CY, SXX, SYY, SXY, SLANT, SPREAD = range(8)
SIZES = (64, 128)
SYY_MIN = _lib.SHAPE_SYY_MIN
N_SUMS = _lib.SHAPE_SUMS


# ---- the numpy fp64 restatement -------------------------------------------------------------------------------------------
def _coordinates(s: int) -> Tuple[np.ndarray, np.ndarray]:
    """(u, v), each (s, s): the coordinates of every pixel of an s x s image, exact in fp64."""
    t = (np.arange(s, dtype=np.float64) + 0.5) / s - 0.5
    v, u = np.meshgrid(t, t, indexing="ij")
    return u, v


def _as_images(images) -> np.ndarray:
    x = np.asarray(images)
    if x.ndim == 4 and x.shape[1] == 1:
        x = x[:, 0]
    if x.ndim != 3 or x.shape[1] != x.shape[2] or x.shape[1] not in SIZES:
        raise ValueError(f"images must be (B, s, s) or (B, 1, s, s) with s in {SIZES}, got {x.shape}")
    return x


def _features_of_ink(a: np.ndarray, reverse: bool = False) -> np.ndarray:
    """The eight features of one fp64 ink image (s, s); ``reverse``: every sum runs over the pixels in descending order."""
    s = a.shape[0]
    u, v = _coordinates(s)
    total = (lambda t: float(np.sum(t.reshape(-1)[::-1]))) if reverse else (lambda t: float(np.sum(t)))
    f = np.zeros(8, dtype=np.float64)
    s0 = total(a)
    f[MASS] = s0 / (s * s)
    if not s0 > 0.0:
        return f
    cx, cy = total(a * u) / s0, total(a * v) / s0
    du, dv = u - cx, v - cy
    f[CX], f[CY] = cx, cy
    f[SXX], f[SYY], f[SXY] = total(a * (du * du)) / s0, total(a * (dv * dv)) / s0, total(a * (du * dv)) / s0
    f[SLANT] = f[SXY] / f[SYY] if f[SYY] > SYY_MIN else 0.0
    f[SPREAD] = f[SXX] + f[SYY]
    return f


def reference_features(images, reverse: bool = False) -> np.ndarray:
    """(B, 8) fp64: the features of fp32 (or fp64) images in [-1, 1] by the definitions, in numpy.  Needs no device."""
    x = _as_images(images).astype(np.float64)
    return np.stack([_features_of_ink((1.0 - img) * 0.5, reverse) for img in x]) if len(x) else np.zeros((0, 8))


def reference_objective(features, weights, targets, s0_positive=None) -> np.ndarray:
    """(B,) fp64: 0.5 * sum_k w_k (f_k - t_k)^2 over the terms that contribute (see the module docstring).  ``s0_positive``
    (B,) bool: which images are not empty (None: mass > 0)."""
    f, w, t = (np.asarray(v, dtype=np.float64).reshape(-1, 8) for v in (features, weights, targets))
    full = np.asarray(f[:, MASS] > 0.0 if s0_positive is None else s0_positive, dtype=bool)
    out = np.zeros(len(f))
    for i in range(len(f)):
        for k in range(8):
            if w[i, k] == 0.0 or (k != MASS and not full[i]) or (k == SLANT and not f[i, SYY] > SYY_MIN):
                continue
            out[i] += 0.5 * w[i, k] * (f[i, k] - t[i, k]) ** 2
    return out


def reference_grad(images, weights, targets) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(dx (B, s, s) fp64, objective (B,) fp64, features (B, 8) fp64): the gradient of reference_objective with respect to the
    PIXELS, term by term as the header states it: dx_p = -0.5 * sum_k w_k (f_k - t_k) df_k/da_p.  Needs no device."""
    x = _as_images(images).astype(np.float64)
    b, s = x.shape[0], x.shape[1]
    w, t = (np.asarray(v, dtype=np.float64).reshape(b, 8) for v in (weights, targets))
    u, v = _coordinates(s)
    feats = reference_features(x)
    dx = np.zeros_like(x)
    full = np.zeros(b, dtype=bool)
    for i in range(b):
        f = feats[i]
        s0 = float(np.sum((1.0 - x[i]) * 0.5))
        full[i] = s0 > 0.0
        res = lambda k: w[i, k] * (f[k] - t[i, k]) if w[i, k] != 0.0 else 0.0          # noqa: E731
        g = np.full((s, s), res(MASS) / (s * s))
        if full[i]:
            du, dv = u - f[CX], v - f[CY]
            d = {CX: du / s0, CY: dv / s0, SXX: (du * du - f[SXX]) / s0, SYY: (dv * dv - f[SYY]) / s0,
                 SXY: (du * dv - f[SXY]) / s0}
            d[SPREAD] = d[SXX] + d[SYY]
            if f[SYY] > SYY_MIN:
                d[SLANT] = (d[SXY] - f[SLANT] * d[SYY]) / f[SYY]
            for k, dk in d.items():
                g = g + res(k) * dk
        dx[i] = -0.5 * g
    return dx, reference_objective(feats, w, t, full), feats


def reference_sums_u8(u8) -> np.ndarray:
    """(B, 6) int64: siggan_shape_u8's sums in numpy.  Needs no device."""
    b8 = _as_images(u8)
    if b8.dtype != np.uint8:
        raise ValueError(f"byte images must be uint8, got {b8.dtype}")
    s = b8.shape[1]
    ink = 255 - b8.astype(np.int64)
    t = 2 * np.arange(s, dtype=np.int64) + 1 - s
    q, p = np.meshgrid(t, t, indexing="ij")
    return np.stack([(ink * k).sum(axis=(1, 2)) for k in (np.ones_like(p), p, q, p * p, q * q, p * q)], axis=1)


def features_from_sums(sums, s: int) -> np.ndarray:
    """(B, 8) fp64 from the (B, 6) int64 sums (S0, Sp, Sq, Spp, Sqq, Spq) of byte images, for ink (255 - b) / 255:
        mass = S0 / (255 s^2);  cx = Sp / (2 s S0);  cy = Sq / (2 s S0);
        sxx = (S0 Spp - Sp^2) / (4 s^2 S0^2);  syy = (S0 Sqq - Sq^2) / (4 s^2 S0^2);  sxy = (S0 Spq - Sp Sq) / (4 s^2 S0^2);
        slant = sxy / syy, or 0 when syy <= 1e-12;  spread = sxx + syy
    -- every numerator an exact int64 (below 2.9e17 at s = 128), converted to fp64 once and divided by the fp64 product
    (4 s^2) * (S0 * S0), S0 converted first.  An image with S0 == 0 has features 1..7 = 0."""
    if s not in SIZES:
        raise ValueError(f"s must be one of {SIZES}, got {s}")
    m = np.asarray(sums)
    if m.dtype != np.int64 or m.ndim != 2 or m.shape[1] != N_SUMS:
        raise ValueError(f"sums must be int64 (B, {N_SUMS}), got {m.dtype} {m.shape}")
    out = np.zeros((m.shape[0], 8), dtype=np.float64)
    for i, (s0, sp, sq, spp, sqq, spq) in enumerate(m):
        out[i, MASS] = np.float64(s0) / (255.0 * s * s)
        if s0 <= 0:
            continue
        s0f = np.float64(s0)
        den = (4.0 * s * s) * (s0f * s0f)
        out[i, CX], out[i, CY] = np.float64(sp) / (2.0 * s * s0f), np.float64(sq) / (2.0 * s * s0f)
        out[i, SXX] = np.float64(s0 * spp - sp * sp) / den
        out[i, SYY] = np.float64(s0 * sqq - sq * sq) / den
        out[i, SXY] = np.float64(s0 * spq - sp * sq) / den
        out[i, SLANT] = out[i, SXY] / out[i, SYY] if out[i, SYY] > SYY_MIN else 0.0
        out[i, SPREAD] = out[i, SXX] + out[i, SYY]
    return out


# ---- the device calls -----------------------------------------------------------------------------------------------------
def _check_images(images, dtype: torch.dtype, what: str) -> Tuple[int, int]:
    """The refusals that need no device, in a fixed order: type, dtype, rank and sizes, device, layout.  Returns (B, s)."""
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{what} must be a tensor, got {type(images).__name__}")
    if images.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {images.dtype}")
    if not (images.dim() == 3 or (images.dim() == 4 and images.shape[1] == 1)):
        raise ValueError(f"{what} must be (B, s, s) or (B, 1, s, s), got {tuple(images.shape)}")
    b, h, w = images.shape[0], images.shape[-2], images.shape[-1]
    if h != w or h not in SIZES:
        raise ValueError(f"{what} must be square with a side in {SIZES}, got {h} x {w}")
    if b < 1:
        raise ValueError(f"{what} holds no image")
    _call.check_resident(images, what)
    return b, h


def _check_rows(name: str, t, b: int, dev: torch.device, weights: bool) -> torch.Tensor:
    """weights / targets -> a contiguous fp64 (B, 8) tensor on ``dev``.  Anything array-like of that shape is taken (a host
    array is validated on the host and copied); a tensor already on the device must be fp64, and weights there are checked
    with one small synchronising reduction -- negative or non-finite weights never reach the kernel."""
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.array(t, dtype=np.float64))             # (a copy: B x 8 numbers; the caller's array may be read-only)
    if tuple(t.shape) != (b, 8):
        raise ValueError(f"{name} must be ({b}, 8), got {tuple(t.shape)}")
    if t.dtype != torch.float64:
        raise ValueError(f"{name} must be float64, got {t.dtype}")
    if t.device.type == "cuda" and t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, the images on {dev}")
    if weights and not bool((torch.isfinite(t) & (t >= 0)).all()):
        raise ValueError(f"{name} must be finite and >= 0")
    return t.to(dev).contiguous()


def _out(name: str, t: Optional[torch.Tensor], shape, dtype: torch.dtype, dev: torch.device) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous()
            or t.numel() != int(np.prod(shape)) or (len(shape) > 1 and tuple(t.shape[-2:]) != tuple(shape[-2:]))
            or (len(shape) == 1 and tuple(t.shape) != tuple(shape))):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor {tuple(shape)} on {dev}")
    return t


def shape_features(images: torch.Tensor) -> torch.Tensor:
    """(B, 8) fp64 on the device: the features (FEATURES) of contiguous fp32 device images (B, 1, s, s) or (B, s, s)."""
    b, s = _check_images(images, torch.float32, "images")
    dev = device_of(images)
    feats = torch.empty(b, 8, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().siggan_shape_f32(dev.index, ptr(images), b, s, None, None, ptr(feats), None, None, stream(dev)))
    return feats


def shape_grad(images: torch.Tensor, weights, targets, dx_out: Optional[torch.Tensor] = None,
               objective_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dx fp32 (B, 1, s, s), objective fp32 (B,), features fp64 (B, 8)), all on the device: the per-image objective
    0.5 * sum_k w_k (f_k - t_k)^2 of contiguous fp32 device images and its gradient with respect to the pixels, one launch.
    ``weights`` / ``targets``: (B, 8) fp64, finite weights >= 0 (host arrays are taken too; weights already on the device cost
    one small synchronising check -- pass a host array, or call the library directly, inside a loop that must not wait).
    ``dx_out`` / ``objective_out``: caller-owned contiguous fp32 device tensors the results are written into."""
    b, s = _check_images(images, torch.float32, "images")
    dev = device_of(images)
    w = _check_rows("weights", weights, b, dev, True)
    t = _check_rows("targets", targets, b, dev, False)
    return _shape_grad_checked(images, b, s, dev, w, t, dx_out, objective_out)


def _shape_grad_checked(images, b, s, dev, w, t, dx_out=None, objective_out=None):
    """shape_grad behind its weight check: what a loop calls every iteration with rows it has validated once."""
    dx = _out("dx_out", dx_out, (b, 1, s, s), torch.float32, dev)
    obj = _out("objective_out", objective_out, (b,), torch.float32, dev)
    feats = torch.empty(b, 8, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().siggan_shape_f32(dev.index, ptr(images), b, s, ptr(w), ptr(t), ptr(feats), ptr(dx), ptr(obj),
                                            stream(dev)))
    return dx, obj, feats


def shape_sums_u8(u8: torch.Tensor) -> torch.Tensor:
    """(B, 6) int64 on the device: sum ink, ink p, ink q, ink p^2, ink q^2, ink p q of contiguous uint8 device images
    (B, s, s) or (B, 1, s, s), exact (ink = 255 - b, p = 2c + 1 - s, q = 2r + 1 - s).  features_from_sums makes features of them."""
    b, s = _check_images(u8, torch.uint8, "byte images")
    dev = device_of(u8)
    sums = torch.empty(b, N_SUMS, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().siggan_shape_u8(dev.index, ptr(u8), b, s, ptr(sums), stream(dev)))
    return sums
