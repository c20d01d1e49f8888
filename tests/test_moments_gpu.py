"""The streaming fp64 feature moments on the MI355X (include/siggan_moments.h, csrc/moments.hip, utils/frechet.py).

Yardstick: the moments of x.astype(float64) in numpy.  Bound, per entry: n_total 2^-52 (|x|^T |x|)_ij on G and
n_total 2^-52 sum_r |x_rj| on s -- the standard dot-product bound gamma_n with a factor 2 (one for each side), which holds
for any summation order; the fp32 -> fp64 conversion and every product of two fp32 values are exact.

Shapes are the smallest at which tiling or tails can go wrong: D = 1 (one lane of one tile), 16 (exactly one tile), 40 (a
partial third tile: 6 tiles of the upper triangle), 128 (8 x 8 tiles with the mirror); n = 1, 3 (inside one K step), 4 (one
full step), 5 (a step and a tail), 67 (16 steps and a tail).  The columns are scaled by factors from 1e-3 to 1e3, so a row or
column that lands in the wrong place is off by orders of magnitude, not by something the bound could hide."""
import ctypes as C

import numpy as np
import pytest
import torch

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils.frechet import FeatureMoments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U2 = 2.0 ** -52


def features(n, d, seed=0):
    rng = np.random.default_rng([seed, n, d])
    scale = 10.0 ** rng.uniform(-3.0, 3.0, d)
    return (rng.standard_normal((n, d)) * scale).astype(np.float32)


def check_moments(got, x, what):
    """got = (count, s, G) of the accumulator after all rows of x went in."""
    n, s, g = got
    x = x.astype(np.float64)
    ax = np.abs(x)
    e_s, b_s = np.abs(s - x.sum(axis=0)), x.shape[0] * U2 * ax.sum(axis=0)
    e_g, b_g = np.abs(g - x.T @ x), x.shape[0] * U2 * (ax.T @ ax)
    print(f"{what}: worst s error / bound {float((e_s / b_s).max()):.3e}, worst G error / bound {float((e_g / b_g).max()):.3e}")
    assert n == x.shape[0]
    assert s.dtype == np.float64 and g.dtype == np.float64 and s.shape == (x.shape[1],) and g.shape == (x.shape[1],) * 2
    assert (e_s <= b_s).all(), f"{what}: sum vector off at {np.argwhere(e_s > b_s)[:4].tolist()}"
    assert (e_g <= b_g).all(), f"{what}: Gram matrix off at {np.argwhere(e_g > b_g)[:4].tolist()}"
    assert np.array_equal(g, g.T), f"{what}: G is not exactly symmetric"


@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])
@pytest.mark.parametrize("d", [1, 16, 40, 128])
def test_one_update(d, n):
    x = features(n, d)
    m = FeatureMoments(d, DEV)
    m.update(torch.from_numpy(x).to(DEV))
    check_moments(m.read(), x, f"D={d} n={n}")
    assert m.count == n
    m.close()


@pytest.mark.parametrize("d", [40, 128])
def test_accumulation_reset_and_determinism(d):
    x = features(73, d, seed=1)
    xd = torch.from_numpy(x).to(DEV)

    def run(m):
        for lo, hi in ((0, 5), (5, 72), (72, 73)):
            m.update(xd[lo:hi])
        return m.read()

    m = FeatureMoments(d, DEV)
    first = run(m)
    check_moments(first, x, f"D={d} 5 + 67 + 1 rows")
    # a second accumulator, the same sequence: the same bits (one owner per tile, a fixed order, no atomics)
    m2 = FeatureMoments(d, DEV)
    second = run(m2)
    assert first[0] == second[0] == 73 and np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    # reset, then one update: what a fresh accumulator gives
    m.reset()
    assert m.count == 0
    n0, s0, g0 = m.read()
    assert n0 == 0 and not s0.any() and not g0.any()
    m.update(xd[5:72])
    fresh = FeatureMoments(d, DEV)
    fresh.update(xd[5:72])
    a, b = m.read(), fresh.read()
    assert a[0] == b[0] == 67 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    check_moments(a, x[5:72], f"D={d} after reset")
    # finish() is the host arithmetic on exactly these moments
    n, mean, cov = m2.finish()
    assert n == 73 and np.array_equal(mean, second[1] / 73) and np.array_equal(cov, cov.T)
    for acc in (m, m2, fresh):
        acc.close()


def test_argument_errors_start_nothing():
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    h = C.c_void_p()
    for dim in (0, 1025):
        assert lib.siggan_moments_create(0, dim, C.byref(h)) == _lib.E_ARG and not h.value
        assert b"dim" in lib.siggan_last_error()
    with pytest.raises(ValueError):
        FeatureMoments(0, DEV)
    x = features(4, 16)
    xd = torch.from_numpy(x).to(DEV)
    m = FeatureMoments(16, DEV)
    m.update(xd)
    before = m.read()
    p = C.c_void_p(xd.data_ptr())
    for n_rows in (0, -2):
        assert lib.siggan_moments_update(m._h, p, n_rows, st) == _lib.E_ARG
        assert b"n_rows" in lib.siggan_last_error()
    assert lib.siggan_moments_update(m._h, None, 4, st) == _lib.E_ARG and b"null" in lib.siggan_last_error()
    assert lib.siggan_moments_update(None, p, 4, st) == _lib.E_ARG
    assert lib.siggan_moments_reset(None, st) == _lib.E_ARG and lib.siggan_moments_read(None, None, None, None, st) == _lib.E_ARG
    for bad in (xd.double(), xd[:, :8], xd.t().contiguous().t(), xd.cpu(), xd.reshape(-1)):   # dtype, width, strides, device, rank
        with pytest.raises(ValueError):
            m.update(bad)
    with pytest.raises(ValueError):
        m.update(xd[:0])                                   # no rows: the library's refusal through the shim
    torch.cuda.synchronize()
    after = m.read()
    assert after[0] == before[0] == 4 and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    one = FeatureMoments(16, DEV)
    one.update(xd[:1])
    with pytest.raises(ValueError, match="at least 2"):
        one.finish()
    assert lib.siggan_moments_destroy(None) == 0
    m.close(), one.close()
