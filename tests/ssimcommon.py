"""Single-scale SSIM restated in numpy, and the images it is tried on.

``ssim_matrix64``  the yardstick: the definition of include/siggan_ssim.h in float64, with the float-rounded taps widened to
                   double (the taps are part of the definition; what is measured is the arithmetic after them).
``ssim_matrix32``  the same statements with every array in float32: what a plain fp32 implementation gives.  Its largest
                   deviation from the yardstick over a set of pairs sets the scale of the GPU tests' bound (``World.bound``).
``ssim_scipy``     an independent formulation: scipy.ndimage.correlate1d along both axes, cropped to the valid region.

``World(h, w)`` holds, per size, two image lists A and B made of the families the tests need (blurred poly-lines on white, all
255, all 0, uniform noise, an inverted image, a copy shifted by one pixel, exact duplicates at other batch indices), the
yardstick matrices over all of them and the bound.  The batch cases are PREFIXES of A and B, so the value of one pair can be
compared across batches.  It is computed once per size and shared."""
import functools

import numpy as np
from scipy import ndimage

import componentscommon as CC

TAPS, SIGMA, HALO = 11, 1.5, 10
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
SIZES = [(11, 12), (12, 12), (16, 16), (40, 52), (64, 64), (64, 128), (128, 128)]
MARGIN = 16.0                                        # the GPU bound is MARGIN x the plain-fp32 restatement's own deviation


def batches(h, w):
    """The (na, nb) of the issue at this size."""
    return [(1, 1), (3, 5), (17, 33)] if h * w <= 64 * 64 else [(5, 7)]


def taps():
    """float32 (11,): exp(-(k - 5)^2 / (2 * 1.5^2)) normalised by the sum in double, rounded to float once."""
    k = np.arange(TAPS, dtype=np.float64) - TAPS // 2
    e = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return (e / e.sum()).astype(np.float32)


def _band(n, dtype):
    """(n - 10, n): row o holds the taps at columns o .. o + 10 -- the valid correlation as a matrix."""
    t = np.zeros((n - HALO, n), dtype=dtype)
    g = taps().astype(dtype)
    for o in range(n - HALO):
        t[o, o:o + TAPS] = g
    return t


def _filter(img, dtype):
    """G * img over the last two axes, valid positions only."""
    th, tw = _band(img.shape[-2], dtype), _band(img.shape[-1], dtype)
    return np.matmul(np.matmul(th, img.astype(dtype)), tw.T)


def _matrix(a, b, dtype):
    a, b = np.asarray(a), np.asarray(b)
    x, y = a.astype(dtype), b.astype(dtype)
    c1, c2, two = dtype(C1), dtype(C2), dtype(2)
    mx, my = _filter(x, dtype), _filter(y, dtype)
    vx, vy = _filter(x * x, dtype) - mx * mx, _filter(y * y, dtype) - my * my
    out = np.empty((len(a), len(b)), dtype=dtype)
    count = dtype((a.shape[-2] - HALO) * (a.shape[-1] - HALO))
    for i in range(len(a)):
        mxy = mx[i] * my
        cov = _filter(x[i] * y, dtype) - mxy
        s = ((two * mxy + c1) * (two * cov + c2)) / ((mx[i] * mx[i] + my * my + c1) * (vx[i] + vy + c2))
        out[i] = s.sum(axis=(-2, -1), dtype=dtype) / count
    assert out.dtype == dtype
    return out


def ssim_matrix64(a, b):
    """float64 (na, nb) of uint8 (na, h, w) against uint8 (nb, h, w)."""
    return _matrix(a, b, np.float64)


def ssim_matrix32(a, b):
    return _matrix(a, b, np.float32)


def ssim64(x, y):
    return float(ssim_matrix64(x[None], y[None])[0, 0])


def ssim_scipy(x, y):
    """One pair, float64: correlate1d along rows and columns, the border it invents cropped away."""
    g = taps().astype(np.float64)

    def f(img):
        full = ndimage.correlate1d(ndimage.correlate1d(img, g, axis=0, mode="constant"), g, axis=1, mode="constant")
        return full[HALO // 2:img.shape[0] - HALO // 2, HALO // 2:img.shape[1] - HALO // 2]
    x, y = x.astype(np.float64), y.astype(np.float64)
    mx, my = f(x), f(y)
    vx, vy, cov = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = ((2 * mx * my + C1) * (2 * cov + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return float(s.mean())


# ------------------------------------------------------------------------------------------------------------- images
def strokes(h, w, seed):
    return CC._strokes(h, w, seed)


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def shifted(img):
    """A copy moved one pixel to the right and one down; the uncovered border is white."""
    out = np.full_like(img, 255)
    out[1:, 1:] = img[:-1, :-1]
    return out


def image_lists(h, w, na=17, nb=33):
    """(A (na, h, w), B (nb, h, w)) uint8.  Every family of the issue within the first 3 of A and 5 of B or shortly after;
    duplicates: B[1] = B[7] = A[0] = A[9], B[2] = A[1] (white), B[3] = A[2] (black), B[6] = A[4]."""
    s0, s1 = strokes(h, w, 100 + h + w), strokes(h, w, 200 + h + w)
    white, black = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    a = [s0, white, black, noise(h, w, 1), s1, 255 - s0, shifted(s0), noise(h, w, 2), shifted(s1), s0]
    b = [noise(h, w, 3), s0, white, black, 255 - s0, shifted(s0), s1, s0, noise(h, w, 1)]
    while len(a) < na:
        a.append(strokes(h, w, 300 + len(a)) if len(a) % 3 else noise(h, w, 300 + len(a)))
    while len(b) < nb:
        b.append(strokes(h, w, 400 + len(b)) if len(b) % 4 else 255 - strokes(h, w, 400 + len(b)))
    return np.stack(a[:na]), np.stack(b[:nb])


class World:
    def __init__(self, h, w):
        self.h, self.w = h, w
        self.na, self.nb = max(p[0] for p in batches(h, w)), max(p[1] for p in batches(h, w))
        self.a, self.b = image_lists(h, w, self.na, self.nb)
        self.ab64, self.aa64 = ssim_matrix64(self.a, self.b), ssim_matrix64(self.a, self.a)
        # the scale of an honest fp32 implementation's error at this size, over every pair the tests score
        self.fp32_deviation = max(float(np.abs(ssim_matrix32(self.a, self.b).astype(np.float64) - self.ab64).max()),
                                  float(np.abs(ssim_matrix32(self.a, self.a).astype(np.float64) - self.aa64).max()))
        self.bound = MARGIN * self.fp32_deviation


@functools.lru_cache(maxsize=None)
def world(h, w):
    return World(h, w)


def first_maximum(matrix, skip_diagonal=False):
    """(best, index) of every row as numpy finds them: the first of equal maxima.  One column with the diagonal skipped: -1."""
    m = np.array(matrix, dtype=np.float32, copy=True)
    if skip_diagonal:
        if m.shape[1] == 1:
            return np.full(m.shape[0], -1.0, np.float32), np.full(m.shape[0], -1, np.int32)
        m[np.arange(m.shape[0]), np.arange(m.shape[0])] = -np.inf
    index = np.argmax(m, axis=1)
    return m[np.arange(m.shape[0]), index], index.astype(np.int32)
