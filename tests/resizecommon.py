"""Pillow's Image.resize(size, Image.BILINEAR) for mode 'L', restated in numpy: the coefficient table (precompute_coeffs +
normalize_coeffs_8bpc, in double and in Pillow's operation order), the horizontal pass into a uint8 intermediate and the
vertical pass, both in 22-bit fixed point.  test_resize_cpu.py proves it against Pillow itself; the GPU tests take Pillow for
the bytes and this file for what Pillow does not hand out: the windows, the double weights (the dense fp64 R of the fp32
paths) and the fp32 weights."""
import math

import numpy as np
from PIL import Image

PRECISION_BITS = 32 - 8 - 2
U = 2.0 ** -24                                              # fp32 unit roundoff


def coefficients(n_in, n_out):
    """(bounds (out, 2) int: window start and length; w (out, ksize) float64: normalised triangle weights, 0 past the window)."""
    scale = float(n_in) / n_out
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), dtype=np.int64)
    w = np.zeros((n_out, ksize), dtype=np.float64)
    ss = 1.0 / filterscale
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        ww = 0.0
        for x in range(xmax):
            v = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - v if v < 1.0 else 0.0
            w[xx, x] = v
            ww += v
        if ww != 0.0:
            for x in range(xmax):
                w[xx, x] /= ww
        bounds[xx] = (xmin, xmax)
    return bounds, w


def quantise(w):
    """normalize_coeffs_8bpc: C's (int) truncates towards zero."""
    return np.where(w < 0, np.trunc(-0.5 + w * (1 << PRECISION_BITS)), np.trunc(0.5 + w * (1 << PRECISION_BITS))).astype(np.int64)


def _pass_u8(a, n_out):
    """Resample the LAST axis of uint8 ``a`` to n_out: int accumulator from 1 << 21, shift by 22, clip to 0 .. 255."""
    bounds, w = coefficients(a.shape[-1], n_out)
    kk = quantise(w)
    out = np.empty(a.shape[:-1] + (n_out,), dtype=np.uint8)
    src = a.astype(np.int64)
    for xx in range(n_out):
        xmin, xmax = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + (src[..., xmin:xmin + xmax] * kk[xx, :xmax]).sum(axis=-1)
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8_ref(a, size=(64, 64)):
    """uint8 (..., H, W) -> uint8 (..., h, w): horizontal pass first, its bytes feed the vertical one; an unchanged axis is
    skipped."""
    h, w = size
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape[-1] != w:
        a = _pass_u8(a, w)
    if a.shape[-2] != h:
        a = np.swapaxes(_pass_u8(np.swapaxes(a, -1, -2), h), -1, -2)
    return np.ascontiguousarray(a)


def pillow_resize(a, size=(64, 64)):
    """The oracle: uint8 (N, H, W) through Image.resize, image by image."""
    h, w = size
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(im, dtype=np.uint8)).resize((w, h), Image.BILINEAR), dtype=np.uint8) for im in a])


def dense(n_in, n_out, dtype=np.float64):
    """R (out, in): the axis map as a matrix of the double weights (or of their fp32 roundings, widened again); the identity
    when the axis does not change (the pass is skipped)."""
    if n_in == n_out:
        return np.eye(n_in, dtype=np.float64)
    bounds, w = coefficients(n_in, n_out)
    r = np.zeros((n_out, n_in), dtype=np.float64)
    for xx in range(n_out):
        xmin, xmax = bounds[xx]
        r[xx, xmin:xmin + xmax] = w[xx, :xmax].astype(dtype).astype(np.float64)
    return r


def ksize(n_in, n_out):
    return int(math.ceil(max(float(n_in) / n_out, 1.0))) * 2 + 1


def contents(kind, shape, seed):
    """Test images: 'random' bytes, 'binary' (0 / 255 blobs), 'ruled' (horizontal and vertical lines of period 7 / 5),
    'strokes' (dark anti-aliased pen lines on white), 'zeros', 'full'."""
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if kind == "binary":
        return np.where(rng.random(shape) < 0.3, 0, 255).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(shape, dtype=np.uint8)
    if kind == "full":
        return np.full(shape, 255, dtype=np.uint8)
    h, w = shape[-2:]
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "ruled":
        a = np.where((yy % 7 == 0) | (xx % 5 == 0), 0, 255).astype(np.uint8)
        return np.broadcast_to(a, shape).copy()
    if kind == "strokes":
        out = np.empty(shape, dtype=np.uint8)
        flat = out.reshape(-1, h, w)
        for i in range(flat.shape[0]):
            ink = np.zeros((h, w))
            for _ in range(3):
                a, b, c = rng.uniform(-1, 1), rng.uniform(0, max(h, 1)), rng.uniform(0.6, 2.0)
                ink = np.maximum(ink, np.clip(1.5 - np.abs(yy - (a * xx + b)) / c, 0, 1))
            flat[i] = np.round(255 * (1 - ink)).astype(np.uint8)
        return out
    raise ValueError(kind)
