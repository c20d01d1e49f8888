"""include/siggan_warp.h restated in numpy, written from the header and independent of the kernel: the control grid, the
draws (through rngcommon.draw_raw), the integer B-spline weights, the one rounding of the weighted sum, the 16.16 base map
and the bilinear byte sample.  Plain formulas: every sum in int64, the division a floor division.  Below it the cases the
GPU tests run, shared with the CPU tests that show the restatement can tell a mistaken generator from the right one."""
import numpy as np

import rngcommon as R

SID_WARP = 0x57415250
CELLS = (8, 16, 32)
MAX_CTRL = 8192
IDENTITY = (65536, 0, 0, 0, 65536, 0)


def max_amp(c):
    return int(np.floor(0.4 * c * 256))


def grid(h, w, c):
    """(gy, gx)"""
    return -(-h // c) + 3, -(-w // c) + 3


def weights(k, c):
    """(4, ...) int64: B0 .. B3 at offset(s) k in a cell of c pixels."""
    k = np.asarray(k, np.int64)
    return np.stack([(c - k) ** 3, 3 * k ** 3 - 6 * c * k ** 2 + 4 * c ** 3, -3 * k ** 3 + 3 * c * k ** 2 + 3 * c * c * k + c ** 3, k ** 3])


def control_points(seed, draw_id, amp, h, w, c, sid=SID_WARP, mutant=None):
    """int64 (2, gy, gx): D[comp][j][i] of one image.  mutant: None, or one of the mistakes test_warp_cpu plants --
    'id_as_index' (the draw id taken as the element index and the group as the counter), 'swap' (components swapped),
    'low_half' (word & 0xFFFF for word >> 16)."""
    gy, gx = grid(h, w, c)
    e = np.arange(2 * gy * gx, dtype=np.uint64)
    if mutant == "id_as_index":
        words = R.draw_raw(seed, e >> np.uint64(2), np.uint64(draw_id), sid)
    else:
        words = R.draw_raw(seed, draw_id, e >> np.uint64(2), sid)
    word = np.take_along_axis(words, (e & np.uint64(3)).astype(np.int64)[:, None], axis=-1)[:, 0].astype(np.int64)
    s = ((word & 0xFFFF) if mutant == "low_half" else (word >> 16)) - 32768
    a = np.clip(np.asarray(amp, np.int64), 0, max_amp(c))
    a = a[::-1] if mutant == "swap" else a
    comp = (np.arange(2 * gy * gx) >= gy * gx).astype(np.int64)
    return ((s * a[comp]) >> 15).reshape(2, gy, gx)                   # numpy's >> on int64 is arithmetic


def displacement(D, h, w, c):
    """int64 (2, h, w): disp = floor((2 S + den) / (2 den)), S the tensor-product B-spline sum of the control points D."""
    D = np.clip(np.asarray(D, np.int64), -MAX_CTRL, MAX_CTRL)
    y, x = np.arange(h), np.arange(w)
    by, bx = weights(y % c, c), weights(x % c, c)                     # (4, h), (4, w)
    cy, cx = y // c, x // c
    S = np.zeros((2, h, w), np.int64)
    for b in range(4):
        for a in range(4):
            S += by[b][None, :, None] * bx[a][None, None, :] * D[:, (cy + b)[:, None], (cx + a)[None, :]]
    den = 36 * c ** 6
    return (2 * S + den) // (2 * den)                                   # floor division


def base_map(affine, h, w):
    """int64 (2, h, w) in Q8: ((a2 + y a1 + x a0) >> 8, (a5 + y a4 + x a3) >> 8), no wrapping."""
    a = [int(v) for v in affine]
    y, x = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
    return np.stack([(a[2] + y * a[1] + x * a[0]) >> 8, (a[5] + y * a[4] + x * a[3]) >> 8])


def sample(img, pos, fill):
    """uint8 (h, w): the bilinear byte sample of img at the Q8 positions pos (2, h, w); a tap outside reads fill."""
    h, w = img.shape
    px, py = pos[0], pos[1]
    x0, fx, y0, fy = px >> 8, px & 255, py >> 8, py & 255

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), fill)

    v = ((256 - fx) * (256 - fy) * tap(x0, y0) + fx * (256 - fy) * tap(x0 + 1, y0) + (256 - fx) * fy * tap(x0, y0 + 1) +
         fx * fy * tap(x0 + 1, y0 + 1) + 32768) >> 16
    return v.astype(np.uint8)


def warp_one(img, seed, draw_id, amp, affine, c, fill, ctrl=None, **mut):
    """(uint8 (h, w), int64 (2, h, w)): one output image and its displacement field."""
    h, w = img.shape
    D = control_points(seed, draw_id, amp, h, w, c, **mut) if ctrl is None else np.asarray(ctrl, np.int64)
    disp = displacement(D, h, w, c)
    return sample(img, base_map(affine, h, w) + disp, fill), disp


def warp_batch(src, seed, draw_ids, amp, affines, c, fill, index=None, ctrl=None):
    """(uint8 (n, h, w), int32 (n, 2, h, w)): output i from source clamp(index[i]) (None: i)."""
    n = len(draw_ids)
    idx = np.arange(n) if index is None else np.clip(np.asarray(index, np.int64), 0, len(src) - 1)
    res = [warp_one(src[idx[i]], seed, int(draw_ids[i]), amp, affines[i], c, fill, None if ctrl is None else ctrl[i]) for i in range(n)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]).astype(np.int32)


# ---- the fold check: how far the source position advances per output pixel ----------------------------------------------------
def min_advance(D, h, w, c):
    """The smallest advance, in Q8, of the source x along a row and of the source y along a column under the identity base
    map: positive means the map folds nowhere along rows and columns."""
    disp = displacement(D, h, w, c)
    px = np.arange(w, dtype=np.int64)[None, :] * 256 + disp[0]
    py = np.arange(h, dtype=np.int64)[:, None] * 256 + disp[1]
    return int(min(np.diff(px, axis=1).min(), np.diff(py, axis=0).min()))


def fold_patterns(gy, gx, amp):
    """The four worst-case control patterns at amplitude amp, each (2, gy, gx): alternating columns, alternating rows, a
    checkerboard and a half-plane step, applied to both components."""
    j, i = np.arange(gy)[:, None], np.arange(gx)[None, :]
    one = [np.where((i + 0 * j) % 2 == 0, amp, -amp), np.where((j + 0 * i) % 2 == 0, amp, -amp), np.where((i + j) % 2 == 0, amp, -amp),
           np.where(i + 0 * j < gx // 2, amp, -amp), np.where(j + 0 * i < gy // 2, amp, -amp)]
    return [np.stack([p, p]).astype(np.int64) for p in one]


# ---- the GPU tests' cases -------------------------------------------------------------------------------------------------------
SHAPES = [(8, 8, 8), (40, 68, 16), (64, 64, 8), (64, 64, 16), (128, 128, 32), (128, 128, 8)]   # (h, w, cell)
DRAWS = [(s, o + k) for s, o, steps in R.SEEDS for k in range(steps)]      # rngcommon.SEEDS read as (seed, draw id)
AFFINE_IDENTITY = IDENTITY


def tilted_affine(h, w):
    """5 degrees of rotation, a slant of 0.1 and a scale of 0.9 about the centre, in 16.16, by the header's definition of the
    base map (written out here, not taken from the package): taps fall outside the image."""
    import math
    rot, k, s = math.radians(5.0), 0.1, 0.9
    cos, sin = math.cos(rot), math.sin(rot)
    m = [(k * sin + cos) / s, -(k * cos - sin) / s, 0.0, -sin / s, cos / s, 0.0]
    cx, cy = (w - 1) * 0.5, (h - 1) * 0.5
    m[2] = cx - m[0] * cx - m[1] * cy
    m[5] = cy - m[3] * cx - m[4] * cy
    return tuple(int(math.floor(v * 65536.0 + 0.5)) for v in m)


def contents(h, w, seed=0):
    """uint8 (5, h, w): paper, full ink, a one-pixel checkerboard, single ink pixels in the four corners, random bytes."""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    corners = np.full((h, w), 255, np.uint8)
    corners[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = 0
    return np.stack([np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), np.where((x + y) % 2 == 0, 0, 255).astype(np.uint8), corners,
                     np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)])
