"""Banded dynamic time warping on column profiles restated in numpy, and the images it is tried on (include/siggan_dtw.h).

``profiles``        the four bytes per column (ink count, first and last ink row, vertical runs), uint8 (n, w, 4).
``dtw_matrix``      the banded recurrence as an anti-diagonal sweep over a padded (na, nb, w + 1, w + 1) int64 table: cell (i, j)
                    lives at [i + 1, j + 1], row and column 0 hold BIG except [0, 0] = 0, so D(0, 0) = d(0, 0) and the first row and
                    column need no special case.  A cell outside the band is never written and stays BIG.  A cell that exists has
                    an existing predecessor, so BIG is never the minimum of one: the result does not depend on its value (asserted).
``dtw_plain``       one pair, a plain double loop over the cells: what the sweep is checked against.
``stroke_images``   a small deterministic image maker: dark poly-lines on white; ``signature_family`` draws one hand's variations
                    of the same lines, kept away from the border so that a copy moved a few pixels sideways loses no ink.
``world(h, w)``     per size, two image lists A and B (strokes, all paper, all ink, sparse noise, duplicates), their profiles and
                    the yardstick matrices per band, computed once and shared; the batch cases are prefixes of A and B."""
import functools

import numpy as np
from PIL import Image, ImageDraw

BIG = 1 << 40
SIZES = [(1, 4), (7, 12), (64, 64), (33, 68), (128, 128)]
BATCHES = [(5, 7), (1, 1), (3, 70)]                   # (na, nb): prefixes of the world's lists
NA, NB = 5, 70
EXTREMES = np.array([[0, 32768, 16384], [32768, 0, 32512], [16384, 32512, 0]], dtype=np.int32)


def default_band(w):
    return max(1, w // 8)


def bands(w):
    """The bands of the issue at this width, without repeats, ascending."""
    return sorted({0, 1, default_band(w), w - 1})


def profiles(u8, threshold=128):
    """uint8 (n, h, w) -> uint8 (n, w, 4): c, t, b, r per column."""
    u8 = np.asarray(u8)
    n, h, w = u8.shape
    ink = u8 < threshold
    some = ink.any(axis=1)
    count = ink.sum(axis=1)
    top = np.where(some, ink.argmax(axis=1), h // 2)
    bottom = np.where(some, h - 1 - ink[:, ::-1].argmax(axis=1), h // 2)
    above = np.concatenate([np.zeros((n, 1, w), dtype=bool), ink[:, :-1]], axis=1)
    runs = (ink & ~above).sum(axis=1)
    return np.stack([count, top, bottom, runs], axis=-1).astype(np.uint8)


def packed(prof):
    """uint8 (n, w, 4) -> uint32 (n, w): c | t << 8 | b << 16 | r << 24."""
    return np.ascontiguousarray(prof).view("<u4")[..., 0]


def local_cost(pa, pb):
    """int64 (na, nb, w, w): d(i, j) of every pair."""
    a, b = np.asarray(pa, dtype=np.int64), np.asarray(pb, dtype=np.int64)
    return np.abs(a[:, None, :, None, :] - b[None, :, None, :, :]).sum(axis=-1)


def dtw_matrix(pa, pb, band):
    """int64 (na, nb): banded DTW of every profile of pa (na, w, 4) with every profile of pb (nb, w, 4)."""
    pa, pb = np.asarray(pa), np.asarray(pb)
    na, nb, w = pa.shape[0], pb.shape[0], pa.shape[1]
    assert pb.shape[1] == w and 0 <= band <= w - 1
    cost = local_cost(pa, pb)
    table = np.full((na, nb, w + 1, w + 1), BIG, dtype=np.int64)
    table[:, :, 0, 0] = 0
    for s in range(2 * w - 1):
        i = np.arange(max(0, s - w + 1), min(w - 1, s) + 1)
        j = s - i
        keep = np.abs(i - j) <= band
        i, j = i[keep], j[keep]
        if i.size:
            best = np.minimum(np.minimum(table[:, :, i, j + 1], table[:, :, i + 1, j]), table[:, :, i, j])
            table[:, :, i + 1, j + 1] = cost[:, :, i, j] + best
    out = table[:, :, w, w]
    assert (out < BIG).all()
    return out


def dtw_plain(a, b, band):
    """One pair of profiles (w, 4): the recurrence cell by cell, cells outside the band absent."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    w = a.shape[0]
    table = {}
    for i in range(w):
        for j in range(max(0, i - band), min(w - 1, i + band) + 1):
            d = int(np.abs(a[i] - b[j]).sum())
            before = [table[c] for c in ((i - 1, j), (i, j - 1), (i - 1, j - 1)) if c in table]
            table[i, j] = d + (min(before) if before else 0)
            assert before or (i, j) == (0, 0)
    return table[w - 1, w - 1]


# ------------------------------------------------------------------------------------------------------------- images
def stroke_image(h, w, seed, margin=4):
    """uint8 (h, w): three dark poly-lines on white, drawn at four times the size and reduced; `margin` pixels of paper on
    the left and right where the width allows it."""
    rng = np.random.default_rng(seed)
    scale = 4
    mx = margin if w >= 4 * margin else 0
    im = Image.new("L", (w * scale, h * scale), 255)
    draw = ImageDraw.Draw(im)
    for _ in range(3):
        pts = [(int(rng.integers(mx * scale, (w - mx) * scale)), int(rng.integers(0, h * scale))) for _ in range(5)]
        draw.line(pts, fill=0, width=int(rng.integers(3, 8)))
    return np.asarray(im.resize((w, h), Image.BILINEAR), dtype=np.uint8).copy()


def stroke_images(h, w, n, seed=0, margin=4):
    return np.stack([stroke_image(h, w, seed + 1000 * k, margin) for k in range(n)])


def signature_family(h, w, n, seed=1, jitter=2, margin=8):
    """uint8 (n, h, w): one hand's variations -- the same three poly-lines with every corner moved by up to `jitter` pixels,
    `margin` pixels of paper on the left and right.  Images this alike are what a pixelwise measure confuses once one of them
    is moved sideways."""
    rng = np.random.default_rng(seed)
    scale = 4
    base = [[(int(rng.integers(margin * scale, (w - margin) * scale)), int(rng.integers(4 * scale, (h - 4) * scale))) for _ in range(5)]
            for _ in range(3)]
    widths = [int(rng.integers(3, 8)) for _ in range(3)]
    out = []
    for _ in range(n):
        im = Image.new("L", (w * scale, h * scale), 255)
        draw = ImageDraw.Draw(im)
        for pts, width in zip(base, widths):
            moved = [(x + int(rng.integers(-jitter * scale, jitter * scale + 1)), y + int(rng.integers(-jitter * scale, jitter * scale + 1)))
                     for x, y in pts]
            draw.line(moved, fill=0, width=width)
        out.append(np.asarray(im.resize((w, h), Image.BILINEAR), dtype=np.uint8).copy())
    return np.stack(out)


def shifted(images, dx):
    """Copies moved dx pixels to the right (left for dx < 0); the uncovered columns are paper."""
    out = np.full_like(images, 255)
    if dx >= 0:
        out[..., dx:] = images[..., :images.shape[-1] - dx]
    else:
        out[..., :dx] = images[..., -dx:]
    return out


def sparse_noise(h, w, seed, p=0.15):
    rng = np.random.default_rng(seed)
    return np.where(rng.random((h, w)) < p, rng.integers(0, 128, (h, w)), rng.integers(128, 256, (h, w))).astype(np.uint8)


def image_lists(h, w, na=NA, nb=NB):
    """(A (na, h, w), B (nb, h, w)) uint8.  A: strokes, paper, ink, noise, strokes.  B: A[0] twice (B[1] = B[4] = A[0]), paper,
    ink, and after that strokes and noise in turn; B[9] = B[1] again."""
    s = [stroke_image(h, w, 10 * h + w + k, margin=0) for k in range(3)]
    paper, inked = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    a = [s[0], paper, inked, sparse_noise(h, w, 1), s[1]]
    b = [s[2], s[0], paper, inked, s[0], sparse_noise(h, w, 2)]
    while len(b) < nb:
        k = len(b)
        b.append(s[0] if k == 9 else (sparse_noise(h, w, 100 + k, 0.05 + 0.01 * (k % 30)) if k % 3 == 0 else stroke_image(h, w, 7000 + 31 * k + w, 0)))
    return np.stack(a[:na]), np.stack(b[:nb])


class World:
    def __init__(self, h, w):
        self.h, self.w = h, w
        self.a, self.b = image_lists(h, w)
        self.pa, self.pb = profiles(self.a), profiles(self.b)

    @functools.lru_cache(maxsize=None)
    def ab(self, band):
        return dtw_matrix(self.pa, self.pb, band).astype(np.int32)

    @functools.lru_cache(maxsize=None)
    def aa(self, band):
        return dtw_matrix(self.pa, self.pa, band).astype(np.int32)


@functools.lru_cache(maxsize=None)
def world(h, w):
    return World(h, w)


def extreme_images():
    """uint8 (3, 128, 128): all ink, all paper, every second row inked."""
    rows = np.full((128, 128), 255, np.uint8)
    rows[0::2] = 0
    return np.stack([np.zeros((128, 128), np.uint8), np.full((128, 128), 255, np.uint8), rows])


def first_minimum(matrix, skip_diagonal=False):
    """(best, index) of every row as numpy finds them: the first of equal minima.  One column with the diagonal skipped: -1."""
    m = np.array(matrix, dtype=np.int64, copy=True)
    if skip_diagonal:
        if m.shape[1] == 1:
            return np.full(m.shape[0], -1, np.int32), np.full(m.shape[0], -1, np.int32)
        m[np.arange(m.shape[0]), np.arange(m.shape[0])] = BIG
    index = np.argmin(m, axis=1)
    return m[np.arange(m.shape[0]), index].astype(np.int32), index.astype(np.int32)
