"""Scan preprocessing restated in numpy / scipy, stage by stage (include/siggan_preprocess.h), and a seeded world of scans.

This file is the definition the kernels of csrc/preprocess.hip are held to, exactly: every stage is integer arithmetic but
for the four doubles of the resize geometry, which are plain Python floats here.  Nothing in it comes from OpenCV; which
stages follow OpenCV's rule as its 4.x source reads and which replace it is tabulated in DESIGN.md.

``restate(g, T, ...)`` runs the pipeline on one (h, w) uint8 scan and returns dict(out, stats, denoised, canvas).
``world()`` is the ragged batch of the GPU tests: random pen strokes on noisy paper at the sizes that make offsets unaligned
and tiles partial, and the planted cases, each under a name."""
import math

import numpy as np
from scipy import ndimage

(STATUS, WHITE, COMPONENTS, KEPT, CROP_X, CROP_Y, CROP_W, CROP_H, NEW_W, NEW_H, SHIFT_X, SHIFT_Y, M00) = range(13)
COUNT = 13
NO_BBOX, DEGENERATE, OVERFLOW = 1, 2, 4
MIN_SIDE, MAX_SIDE, MAX_MARGIN = 16, 1024, 64
MAX_NOISE_RATIO, MIN_INK_RATIO, MIN_CONTOUR_AREA_RATIO = 0.95, 0.01, 0.001      # the reference's constants
EIGHT = np.ones((3, 3), dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------- stage 1
def blur(g):
    """(sum k[dy] k[dx] g + 8) >> 4, k = (1, 2, 1), reflection without the edge (-1 -> 1, n -> n - 2)."""
    p = np.pad(g.astype(np.int64), 1, mode="reflect")
    rows = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    return ((rows[:-2] + 2 * rows[1:-1] + rows[2:] + 8) >> 4).astype(np.uint8)


def three(a, op):
    """op over a at (y - 1, x), (y, x - 1), (y, x); positions outside the image are skipped."""
    r = a.copy()
    r[1:] = op(r[1:], a[:-1])
    r[:, 1:] = op(r[:, 1:], a[:, :-1])
    return r


def denoise(g):
    return three(three(blur(g), np.minimum), np.maximum)


# ------------------------------------------------------------------------------------------------------------- stage 2
def is_valid(white, total):
    """The reference's decision, with its own expressions."""
    dark = total - white
    white_ratio = white / total
    ink_ratio = dark / total
    if white_ratio > MAX_NOISE_RATIO:
        return False
    if ink_ratio < MIN_INK_RATIO:
        return False
    return True


# ------------------------------------------------------------------------------------------------------------- stage 3
def min_pixels(h, w):
    """The smallest integer n with n > h * w * 0.001 as a Python float."""
    return math.floor(h * w * MIN_CONTOUR_AREA_RATIO) + 1


def crop_box(d, min_px, margin):
    """(components, kept, (x, y, cw, ch) or None)."""
    h, w = d.shape
    lab, comps = ndimage.label(d <= 127, structure=EIGHT)
    if comps == 0:
        return 0, 0, None
    counts = np.bincount(lab.ravel(), minlength=comps + 1)
    keep = counts >= min_px
    keep[0] = False
    kept = int(keep.sum())
    if kept == 0:
        return comps, 0, None
    ys, xs = np.nonzero(keep[lab])
    x0, y0, bw, bh = int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
    x = max(0, x0 - margin)
    y = max(0, y0 - margin)
    cw = min(w - x, bw + 2 * margin)
    ch = min(h - y, bh + 2 * margin)
    return comps, kept, (x, y, cw, ch)


# ------------------------------------------------------------------------------------------------------------- stage 4
def resize_geometry(cw, ch, T):
    scale = min(T / cw, T / ch)
    return int(cw * scale), int(ch * scale)


def overlaps(n_src, n_dst):
    """(n_dst, n_src) int64: the length, in units of 1 / n_dst of a source pixel, that source pixel x shares with output X."""
    x = np.arange(n_src, dtype=np.int64)[None, :]
    X = np.arange(n_dst, dtype=np.int64)[:, None]
    return np.clip(np.minimum((x + 1) * n_dst, (X + 1) * n_src) - np.maximum(x * n_dst, X * n_src), 0, None)


def box_resample(c, nw, nh):
    ch, cw = c.shape
    acc = overlaps(ch, nh) @ c.astype(np.int64) @ overlaps(cw, nw).T
    return ((acc + ((cw * ch) >> 1)) // (cw * ch)).astype(np.uint8)


def paste(r, T):
    nh, nw = r.shape
    canvas = np.full((T, T), 255, dtype=np.uint8)
    xo, yo = (T - nw) // 2, (T - nh) // 2
    canvas[yo:yo + nh, xo:xo + nw] = r
    return canvas


# ------------------------------------------------------------------------------------------------------------- stage 5
def centre(canvas):
    """(centred, shift_x, shift_y, m00)."""
    T = canvas.shape[0]
    inv = 255 - canvas.astype(np.int64)
    m00 = int(inv.sum())
    if m00 == 0:
        return canvas.copy(), 0, 0, 0
    m10 = int((inv * np.arange(T)[None, :]).sum())
    m01 = int((inv * np.arange(T)[:, None]).sum())
    sx, sy = T // 2 - m10 // m00, T // 2 - m01 // m00
    out = np.full_like(canvas, 255)
    ys, xs = np.arange(T)[:, None] - sy, np.arange(T)[None, :] - sx
    ok = (ys >= 0) & (ys < T) & (xs >= 0) & (xs < T)
    out[ok] = canvas[np.clip(ys, 0, T - 1), np.clip(xs, 0, T - 1)][ok]
    return out, sx, sy, m00


# ------------------------------------------------------------------------------------------------------------- stage 6
def round_half_even_div(num, den):
    num = np.asarray(num, dtype=np.int64)
    q, r = num // den, num % den
    return q + ((2 * r > den) | ((2 * r == den) & (q % 2 == 1)))


def clahe_lut(tile_pixels, clip):
    """The 256-entry LUT of one tile."""
    a = tile_pixels.size
    hist = np.bincount(tile_pixels.ravel(), minlength=256).astype(np.int64)
    clipped = int(np.maximum(hist - clip, 0).sum())
    hist = np.minimum(hist, clip)
    batch = clipped // 256
    residual = clipped - 256 * batch
    hist += batch
    if residual > 0:
        step = max(256 // residual, 1)
        hist[np.arange(residual) * step] += 1
    return np.minimum(round_half_even_div(np.cumsum(hist) * 255, a), 255)


def clahe(img):
    T = img.shape[0]
    t = T // 8
    a = t * t
    clip = max(int(2.0 * a / 256), 1)
    luts = np.stack([np.stack([clahe_lut(img[ty * t:(ty + 1) * t, tx * t:(tx + 1) * t], clip) for tx in range(8)]) for ty in range(8)])
    n = 2 * np.arange(T) - t                         # (y / t - 0.5) in units of 1 / (2 t)
    t1 = n // (2 * t)                                # floor
    wa = n - t1 * 2 * t                              # the weight of tile t1 + 1, in 0 .. 2 t - 1
    wb = 2 * t - wa
    i1, i2 = np.clip(t1, 0, 7), np.clip(t1 + 1, 0, 7)
    v = img.astype(np.intp)
    Y1, Y2, X1, X2 = i1[:, None], i2[:, None], i1[None, :], i2[None, :]
    ya, yb, xa, xb = wa[:, None], wb[:, None], wa[None, :], wb[None, :]
    top = luts[Y1, X1, v] * xb + luts[Y1, X2, v] * xa
    bot = luts[Y2, X1, v] * xb + luts[Y2, X2, v] * xa
    return round_half_even_div(top * yb + bot * ya, 4 * a).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ pipeline
def restate(g, T=64, denoise_on=True, crop=True, center=True, equalize=True, margin=5, min_px=None):
    assert g.dtype == np.uint8 and g.ndim == 2 and T in (64, 128)
    h, w = g.shape
    stats = np.zeros(COUNT, dtype=np.int32)
    d = denoise(g) if denoise_on else g.copy()
    stats[WHITE] = int((d > 127).sum())
    x, y, cw, ch = 0, 0, w, h
    if crop:
        comps, kept, box = crop_box(d, min_pixels(h, w) if min_px is None else min_px, margin)
        stats[COMPONENTS], stats[KEPT] = comps, kept
        if box is None:
            stats[STATUS] |= NO_BBOX
        else:
            x, y, cw, ch = box
    stats[CROP_X:CROP_H + 1] = (x, y, cw, ch)
    nw, nh = resize_geometry(cw, ch, T)
    if nw < 1 or nh < 1:
        stats[STATUS] |= DEGENERATE
        blank = np.full((T, T), 255, dtype=np.uint8)
        return dict(out=blank, stats=stats, denoised=d, canvas=blank.copy())
    stats[NEW_W], stats[NEW_H] = nw, nh
    canvas = paste(box_resample(d[y:y + ch, x:x + cw], nw, nh), T)
    if center:
        canvas, stats[SHIFT_X], stats[SHIFT_Y], stats[M00] = centre(canvas)
    out = clahe(canvas) if equalize else canvas.copy()
    return dict(out=out, stats=stats, denoised=d, canvas=canvas)


def validity(stats, geom):
    """bool per scan: stage 2's decision from the WHITE column and the (n, 4) geometry {offset, height, width, min_pixels}."""
    return np.array([is_valid(int(s[WHITE]), int(g[1]) * int(g[2])) for s, g in zip(np.asarray(stats), np.asarray(geom))], dtype=bool)


# --------------------------------------------------------------------------------------------------------------- world
RANDOM_SIZES = [(16, 16), (17, 23), (64, 64), (65, 130), (200, 333), (48, 80), (96, 61), (131, 257), (40, 200), (222, 97), (64, 192), (75, 75)]


def pen_scan(h, w, seed, min_ink=0.09):
    """Pen strokes (PIL polylines of varying width, grey ink) on noisy paper with dark specks, until `min_ink` of the pixels is ink."""
    from PIL import Image, ImageDraw
    rng = np.random.RandomState(seed)
    im = Image.new("L", (w, h), 255)
    draw = ImageDraw.Draw(im)
    lo_x, hi_x, lo_y, hi_y = w // 6, w - w // 6, h // 5, h - h // 5
    for _ in range(400):
        pts = [(int(rng.randint(lo_x, hi_x + 1)), int(rng.randint(lo_y, hi_y + 1))) for _ in range(int(rng.randint(3, 7)))]
        draw.line(pts, fill=int(rng.randint(10, 100)), width=int(rng.randint(1, max(2, min(h, w) // 10) + 1)))
        if (np.asarray(im) <= 127).mean() >= min_ink:
            break
    a = np.asarray(im).astype(np.int64)
    paper = 238 + rng.randint(-17, 18, size=(h, w))
    a = np.where(a < 255, a + rng.randint(-8, 9, size=(h, w)), paper)
    specks = rng.rand(h, w) < 0.004
    a = np.where(specks, rng.randint(0, 120, size=(h, w)), a)
    return np.clip(a, 0, 255).astype(np.uint8)


def comb(n):
    a = np.full((n, n), 255, dtype=np.uint8)
    a[n - 3:n - 1, 2:n - 2] = 0                      # the spine at the bottom: the teeth meet late in raster order
    a[2:n - 1, 2:n - 2:2] = 0
    return a


def spiral(n):
    a = np.full((n, n), 255, dtype=np.uint8)
    y = x = 1
    dy, dx = 0, 1
    length = n - 3
    a[y, x] = 0
    while length > 0:
        for _ in range(2):
            for _ in range(length):
                y, x = y + dy, x + dx
                a[y, x] = 0
            dy, dx = dx, -dy
        length -= 2
    return a


def planted():
    """name -> scan.  What each is for stands beside it; the properties hold as planted with denoise off."""
    rng = np.random.RandomState(2024)
    out = {}
    out["blank"] = (248 + rng.randint(-4, 5, size=(64, 64))).astype(np.uint8)                  # no ink at all: NO_BBOX, invalid
    a = np.full((100, 100), 255, dtype=np.uint8)                                                  # min_pixels = 11
    for k in range(6):
        a[10 + 12 * k:12 + 12 * k, 10:15] = 0                                                     # six specks of 10 pixels
    a[30:32, 40:45] = 0
    a[32, 40] = 0                                                                                 # one component of exactly 11
    out["specks"] = a
    a = np.full((64, 64), 255, dtype=np.uint8)
    a[10:15, 10:15] = 0
    a[15:20, 15:20] = 0                                                                           # joined only by the diagonal
    out["diagonal"] = a
    out["comb"] = comb(300)
    out["spiral"] = spiral(300)
    a = np.full((90, 70), 255, dtype=np.uint8)
    a[:, 33:37] = 30
    a[43:47, :] = 60                                                                              # a cross touching all four borders
    out["borders"] = a
    for name, (sy, sx) in {"corner_tl": (slice(0, 20), slice(0, 24)), "corner_tr": (slice(0, 20), slice(-24, None)),
                           "corner_bl": (slice(-20, None), slice(0, 24)), "corner_br": (slice(-20, None), slice(-24, None))}.items():
        a = np.full((80, 100), 255, dtype=np.uint8)
        a[sy, sx] = 40
        out[name] = a
    a = np.full((64, 96), 128, dtype=np.uint8)
    a[:, ::2] = 127
    a[20:40, 30:60] = np.where(rng.rand(20, 30) < 0.5, 127, 128)                                  # bytes 127 and 128 side by side
    out["threshold"] = a
    a = np.full((40, 40), 240, dtype=np.uint8)
    a[14:23, 12:24] = 50                                                                          # a crop smaller than 64: upscaling
    out["small_crop"] = a
    out["texture"] = rng.randint(0, 256, size=(128, 128)).astype(np.uint8)                        # every byte value
    a = np.full((16, 1024), 250, dtype=np.uint8)
    a[7:9, :] = 20                                                                                # crop on: DEGENERATE; off: one pixel high
    out["wide_line"] = a
    a = (rng.randint(0, 256, size=(1024, 16))).astype(np.uint8)
    out["tall_texture"] = a
    return out


_WORLD = None


def world():
    """[(name, scan)], computed once, read-only: the random scans at RANDOM_SIZES, the planted cases, one 1024 x 1024 scan."""
    global _WORLD
    if _WORLD is None:
        items = [(f"pen_{h}x{w}", pen_scan(h, w, 100 + i)) for i, (h, w) in enumerate(RANDOM_SIZES)]
        items += list(planted().items())
        items.append(("pen_1024x1024", pen_scan(1024, 1024, 7, min_ink=0.06)))
        for _, a in items:
            a.setflags(write=False)
        _WORLD = items
    return _WORLD


def is_random(name):
    return name.startswith("pen_")


_EXPECTED = {}


def expected(T=64, denoise_on=True, crop=True, center=True, equalize=True, margin=5):
    """[restate(scan) for every scan of world()], computed once per configuration and left unchanged."""
    key = (T, denoise_on, crop, center, equalize, margin)
    if key not in _EXPECTED:
        res = [restate(a, T, denoise_on, crop, center, equalize, margin) for _, a in world()]
        for r in res:
            for v in r.values():
                v.setflags(write=False)
        _EXPECTED[key] = res
    return _EXPECTED[key]
