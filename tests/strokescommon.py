"""Stroke geometry of byte images restated in numpy, and the images it is tried on (include/siggan_strokes.h).

``reference``   the yardstick of every device output: the border rule by padding with one background pixel, D2 as
                scipy.ndimage.distance_transform_edt squared and rounded, the Guo-Hall passes as whole-array boolean algebra
                on shifted copies, the counters and the disc dilation.  Nothing is shared with the kernel: no row words, no
                column scan, no bit-sliced counters.
``fills``       the random fillings of a shape: Bernoulli ink at 0.1 / 0.5 / 0.9, thresholded blurred noise, Pillow polylines and
                ellipses of pen width 1..7.
``edges``       the edge images: no ink, all ink, corner pixels, the 2 x 2 block, border lines, a checkerboard, bytes on both
                sides of the threshold.
Every result is cached by the image's bytes, so a reference is computed once however many tests ask for it."""
import numpy as np
from PIL import Image, ImageDraw
from scipy import ndimage

INK, SKELETON, ENDPOINTS, JUNCTION_PIXELS, PASSES, D2_MAX, D2_SKEL_SUM, WIDTH_HIST = range(8)
WIDTH_BINS = 16
COUNT = WIDTH_HIST + WIDTH_BINS
GPU_SHAPES = [(1, 4), (2, 4), (3, 8), (5, 12), (33, 64), (64, 64), (64, 68), (128, 4), (127, 124), (128, 128)]
RADII2 = (0, 1, 2, 4, 9, 16, 36)
EIGHT = np.ones((3, 3), dtype=int)
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------- yardstick
def distance2(mask):
    """int (h, w): the squared Euclidean distance of every ink pixel to the nearest background pixel, outside included."""
    d = ndimage.distance_transform_edt(np.pad(mask, 1))[1:-1, 1:-1]
    return np.rint(d * d).astype(np.int64)


def _neighbours(m):
    """P2 .. P9 of a padded boolean array: clockwise from north, north being the row above."""
    p2, p6 = np.roll(m, 1, 0), np.roll(m, -1, 0)
    p4, p8 = np.roll(m, -1, 1), np.roll(m, 1, 1)
    return p2, np.roll(p2, -1, 1), p4, np.roll(p6, -1, 1), p6, np.roll(p6, 1, 1), p8, np.roll(p2, 1, 1)


def thin(mask):
    """Guo-Hall A1 -> (skeleton bool (h, w), passes): the pass that deletes nothing is counted."""
    m = np.pad(mask.astype(bool), 1)                             # the ring stays background: only ink is ever deleted
    passes = 0
    while True:
        changed = False
        for sub in (0, 1):
            p2, p3, p4, p5, p6, p7, p8, p9 = _neighbours(m)
            c = (~p2 & (p3 | p4)).astype(int) + (~p4 & (p5 | p6)) + (~p6 & (p7 | p8)) + (~p8 & (p9 | p2))
            n1 = (p9 | p2).astype(int) + (p3 | p4) + (p5 | p6) + (p7 | p8)
            n2 = (p2 | p3).astype(int) + (p4 | p5) + (p6 | p7) + (p8 | p9)
            n = np.minimum(n1, n2)
            third = ((p2 | p3 | ~p5) & p4) if sub == 0 else ((p6 | p7 | ~p9) & p8)
            delete = m & (c == 1) & (n >= 2) & (n <= 3) & ~third
            if delete.any():
                changed = True
                m = m & ~delete
        passes += 1
        if not changed:
            return m[1:-1, 1:-1].copy(), passes


def width_bins(d2):
    """k in 1..16 per value: the smallest k with d2 <= k * k, 16 above 15 * 15 -- by comparison with the squares."""
    return np.minimum(np.searchsorted(np.arange(0, 70) ** 2, d2, side="left"), WIDTH_BINS)


def counters(mask, skel, passes, d2):
    s = np.zeros(COUNT, dtype=np.int32)
    p2, p3, p4, p5, p6, p7, p8, p9 = (p[1:-1, 1:-1] for p in _neighbours(np.pad(skel, 1)))
    ring = [p2, p3, p4, p5, p6, p7, p8, p9, p2]
    neighbours = sum(r.astype(int) for r in ring[:8])
    transitions = sum((~a & b).astype(int) for a, b in zip(ring[:8], ring[1:]))
    s[INK], s[SKELETON], s[PASSES] = mask.sum(), skel.sum(), passes
    s[ENDPOINTS] = (skel & (neighbours == 1)).sum()
    s[JUNCTION_PIXELS] = (skel & (transitions >= 3)).sum()
    s[D2_MAX] = d2.max() if mask.any() else 0
    s[D2_SKEL_SUM] = d2[skel].sum()
    s[WIDTH_HIST:] = np.bincount(width_bins(d2[skel]), minlength=WIDTH_BINS + 1)[1:]
    return s


def dilate(skel, radius2):
    """bool (h, w): a skeleton pixel within squared distance radius2, clipped to the image."""
    h, w = skel.shape
    r = int(np.sqrt(radius2)) + 1
    out = np.zeros_like(skel)
    padded = np.pad(skel, r)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dy * dy + dx * dx <= radius2:
                out |= padded[r + dy:r + dy + h, r + dx:r + dx + w]
    return out


def geometry(img, threshold=128):
    """(mask, stats (23,) int32, d2 (h, w) int16, skel (h, w) uint8), cached."""
    key = (img.shape, img.tobytes(), threshold)
    if key not in _CACHE:
        mask = img < threshold
        d2 = distance2(mask)
        skel, passes = thin(mask)
        out = (mask, counters(mask, skel, passes, d2), d2.astype(np.int16), skel.astype(np.uint8))
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def reference(img, threshold=128, radius2=0, ink=0, fill=255):
    """-> (stats, d2, skel, redraw) in the layout of include/siggan_strokes.h."""
    _, stats, d2, skel = geometry(img, threshold)
    return stats, d2, skel, np.where(dilate(skel.astype(bool), radius2), ink, fill).astype(np.uint8)


def components8(mask):
    return int(ndimage.label(mask, structure=EIGHT)[1])


# -------------------------------------------------------------------------------------------------------------- cases
def render(ink, threshold, seed):
    """A bool ink mask as bytes: ink anywhere in [0, threshold), background anywhere in [threshold, 255]."""
    rng = np.random.default_rng(seed)
    return np.where(ink, rng.integers(0, threshold, ink.shape), rng.integers(threshold, 256, ink.shape)).astype(np.uint8)


def pillow_strokes(h, w, pen, seed):
    """Two polylines and an ellipse of pen width ``pen``, drawn by Pillow at the image's own size: uint8, ink 0 on 255."""
    rng = np.random.default_rng(seed)
    im = Image.new("L", (w, h), 255)
    d = ImageDraw.Draw(im)
    for _ in range(2):
        d.line([(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(4)], fill=0, width=pen)
    x0, y0 = int(rng.integers(0, max(1, w // 2))), int(rng.integers(0, max(1, h // 2)))
    x1, y1 = x0 + int(rng.integers(1, max(2, w // 2))), y0 + int(rng.integers(1, max(2, h // 2)))
    d.ellipse((x0, y0, x1, y1), outline=0, width=max(1, pen // 2))
    return np.asarray(im, dtype=np.uint8).copy()


def fills(h, w, threshold=128):
    """{name: uint8 (h, w)}: the random fillings of the shape, the same at every call."""
    key = ("fills", h, w, threshold)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * h + w)
        out = {}
        for p in (0.1, 0.5, 0.9):
            out[f"bernoulli_{p}"] = render(rng.random((h, w)) < p, threshold, 3 * h + w)
        blur = ndimage.gaussian_filter(rng.random((h, w)), 1.5)
        out["blurred_noise"] = render(blur > np.quantile(blur, 0.6), threshold, 5 * h + w)
        for pen in range(1, 8):
            out[f"pillow_pen_{pen}"] = pillow_strokes(h, w, pen, 7 * h + w + pen)
        for a in out.values():
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def bar(width, h=64, w=64):
    """An axis-aligned bar of `width` rows and 48 columns, away from the border: ink 0 on 255."""
    g = np.full((h, w), 255, dtype=np.uint8)
    g[20:20 + width, 8:56] = 0
    return g


def edges(h, w, threshold=128):
    """{name: uint8 (h, w)}: the edge images at this shape."""
    yy, xx = np.mgrid[0:h, 0:w]
    z = lambda: np.zeros((h, w), dtype=bool)                     # noqa: E731
    out = {"no_ink": z(), "all_ink": ~z(), "checkerboard": (yy + xx) % 2 == 0}
    for name, (y, x) in {"corner_nw": (0, 0), "corner_ne": (0, w - 1), "corner_sw": (h - 1, 0), "corner_se": (h - 1, w - 1)}.items():
        g = z(); g[y, x] = True
        out[name] = g
    g = z(); g[h // 2:h // 2 + 2, w // 2:w // 2 + 2] = True
    out["block_2x2"] = g
    g = z(); g[0, :] = True
    out["line_north"] = g
    g = z(); g[h - 1, :] = True
    out["line_south"] = g
    g = z(); g[:, 0] = True
    out["line_west"] = g
    g = z(); g[:, w - 1] = True
    out["line_east"] = g
    imgs = {k: render(v, threshold, i) for i, (k, v) in enumerate(out.items())}
    imgs["threshold_bytes"] = np.where((yy + xx // 2) % 3 == 0, threshold - 1, threshold).astype(np.uint8)
    imgs["grey_ramp"] = ((yy * w + xx) % 256).astype(np.uint8)
    return imgs


def mixed_batch(h=64, w=64, n=37):
    """n images of one shape: the fillings and the edge images in turn."""
    pool = list(fills(h, w).values()) + list(edges(h, w).values())
    return np.stack([pool[i % len(pool)] for i in range(n)])
