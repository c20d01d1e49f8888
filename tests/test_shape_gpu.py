"""The shape attributes on the GPU: siggan_shape_f32 / siggan_shape_u8 through shape.py against the numpy fp64 restatement.

Sizes: s = 64 and 128 (the two kernels), B = 1, 5 and 300 (more workgroups than the device has compute units).  One pool of
300 regular images per size and its restated features, gradient and objective are built once and sliced: images do not
interact, so a batch's reference is a slice of the pool's.

Tolerances.  Features, absolute 1e-9: an fp64 sum of n <= 16 384 terms is within n * 2^-53 = 1.8e-12 (relative to S0) of the
exact sum whatever its order, slant divides by syy >= 1e-3, and test_shape_cpu shows 1e-11 for a reordering.  dx, per image
2^-22 of the largest |dx| against the restatement rounded to fp32: one rounding (2^-24 relative) plus the coefficients' fp64
error.  Objective, 1e-6 relative: one fp32 rounding is 6e-8."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import shapecommon as SC
from latentcommon import P_LATENT, P_SIZE, projection_case

pytestmark = pytest.mark.gpu
BATCHES, POOL = (1, 5, 300), 300
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def pool(s):
    """(images fp32 (POOL, s, s), weights, targets, dx fp64, objective fp64, features fp64) -- read-only, shared."""
    from signature_gan_amd import shape as S
    x = SC.regular_images(POOL, s)
    f = S.reference_features(x)
    w, t = SC.objective_rows(POOL, f)
    dx, obj, feats = S.reference_grad(x, w, t)
    for a in (x, w, t, dx, obj, feats):
        a.setflags(write=False)
    return x, w, t, dx, obj, feats


def batch_of(s, b):
    return tuple(a[POOL - b:] for a in pool(s))                                    # (the slanted bar is the last image)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                   # (a copy: the pool is read-only)


@pytest.mark.parametrize("b", BATCHES)
@pytest.mark.parametrize("s", SC.SIZES)
def test_features_gradient_and_objective_against_the_restatement(s, b):
    from signature_gan_amd import shape as S
    x, w, t, dx_ref, obj_ref, f_ref = batch_of(s, b)
    xd = dev(x).unsqueeze(1)
    feats = S.shape_features(xd)
    dx, obj, feats2 = S.shape_grad(xd, w, t)
    assert dx.shape == (b, 1, s, s) and dx.dtype == torch.float32 and obj.shape == (b,) and feats.shape == (b, 8)
    assert torch.equal(feats, feats2)                                              # with or without the gradient: the same bits
    f_err = float(np.abs(feats.cpu().numpy() - f_ref).max())
    want = dx_ref.astype(np.float32)
    scale = np.abs(dx_ref).reshape(b, -1).max(axis=1)
    dx_err = float((np.abs(dx.cpu().numpy()[:, 0].astype(np.float64) - want.astype(np.float64)).reshape(b, -1).max(axis=1) / scale).max())
    obj_err = float((np.abs(obj.cpu().numpy().astype(np.float64) - obj_ref) / np.abs(obj_ref)).max())
    print(f"s = {s}, B = {b}: features {f_err:.2e} (1e-9), dx {dx_err:.2e} of max |dx| (2^-22 = {2.0 ** -22:.2e}), objective {obj_err:.2e} (1e-6)")
    assert f_err <= 1e-9
    assert dx_err <= 2.0 ** -22
    assert obj_err <= 1e-6
    # (B, s, s) without the channel axis is the same call
    assert torch.equal(S.shape_features(dev(x)), feats)


@pytest.mark.parametrize("s", SC.SIZES)
def test_degenerate_images_give_the_stated_exact_values(s):
    from signature_gan_amd import shape as S
    x = np.stack([SC.blank(s), SC.corner_pixel(s), SC.ink_row(s), SC.all_ink(s)])
    w = np.ones((4, 8))
    t = np.full((4, 8), 0.25)
    dx, obj, feats = S.shape_grad(dev(x), w, t)
    f, dx, obj = feats.cpu().numpy(), dx.cpu().numpy()[:, 0], obj.cpu().numpy()
    # blank: every feature 0, dx the uniform mass term, the objective the mass term
    assert np.all(f[0] == 0.0)
    assert np.all(dx[0] == np.float32(-0.5 * (1.0 * (0.0 - 0.25)) / (s * s)))
    assert obj[0] == np.float32(0.5 * 0.25 * 0.25)
    # corner pixel: the centre is the pixel's, the central moments are exactly 0, no slant
    c = -(0.5 - 0.5 / s)
    assert f[1, S.MASS] == 1.0 / (s * s) and f[1, S.CX] == c and f[1, S.CY] == c
    assert np.all(f[1, S.SXX:] == 0.0)
    # ink row: syy is exactly 0, so no slant
    assert f[2, S.SYY] == 0.0 and f[2, S.SLANT] == 0.0 and f[2, S.CX] == 0.0 and f[2, S.MASS] == 1.0 / s
    # all ink: centred; the moments are those of the restatement
    ref = S.reference_features(x)
    assert f[3, S.MASS] == 1.0 and f[3, S.CX] == 0.0 and f[3, S.CY] == 0.0 and f[3, S.SXY] == 0.0 and f[3, S.SLANT] == 0.0
    assert np.abs(f - ref).max() <= 1e-15
    # no slant contribution where there is no slant: the slant's weight and target change no bit (NaN would show)
    w2, t2 = w.copy(), t.copy()
    w2[:3, S.SLANT], t2[:3, S.SLANT] = 7.0, np.nan
    dx2, obj2, _ = S.shape_grad(dev(x), w2, t2)
    assert np.array_equal(dx2.cpu().numpy()[:3, 0], dx[:3]) and np.array_equal(obj2.cpu().numpy()[:3], obj[:3])
    # on the blank image only the mass term is looked at
    t3 = t.copy()
    t3[0, 1:] = np.nan
    dx3, obj3, _ = S.shape_grad(dev(x), w, t3)
    assert np.array_equal(dx3.cpu().numpy()[0, 0], dx[0]) and obj3.cpu().numpy()[0] == obj[0]
    # and the restatement agrees on all four
    dx_ref, obj_ref, _ = S.reference_grad(x, w, t)
    scale = np.abs(dx_ref).reshape(4, -1).max(axis=1)
    assert ((np.abs(dx - dx_ref.astype(np.float32)).reshape(4, -1).max(axis=1) / scale) <= 2.0 ** -22).all()
    assert (np.abs(obj - obj_ref) <= 1e-6 * np.abs(obj_ref)).all()


@pytest.mark.parametrize("s", SC.SIZES)
def test_zero_weight_skips_the_feature_and_its_target(s):
    from signature_gan_amd import shape as S
    x, w, t, *_ = batch_of(s, 5)
    w, t = w.copy(), t.copy()
    w[:, [S.SXX, S.SLANT]] = 0.0
    w[2] = 0.0
    want_dx, want_obj, _ = S.shape_grad(dev(x), w, t)
    t[:, [S.SXX, S.SLANT]] = np.nan
    t[2] = np.nan
    dx, obj, _ = S.shape_grad(dev(x), w, t)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(obj).all())
    assert torch.equal(dx, want_dx) and torch.equal(obj, want_obj)
    assert bool((dx[2] == 0).all()) and float(obj[2]) == 0.0


@pytest.mark.parametrize("s", SC.SIZES)
def test_equal_bits_on_repetition_and_under_a_permutation_of_the_batch(s):
    from signature_gan_amd import shape as S
    x, w, t, *_ = batch_of(s, POOL)
    first = S.shape_grad(dev(x), w, t)
    again = S.shape_grad(dev(x), w, t)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    perm = np.random.default_rng(11).permutation(POOL)
    moved = S.shape_grad(dev(x[perm]), w[perm], t[perm])
    index = torch.from_numpy(perm).to(DEV)
    for a, b in zip(first, moved):
        assert torch.equal(a[index], b)
    u8 = dev(np.random.default_rng(12).integers(0, 256, size=(POOL, s, s), dtype=np.uint8))
    sums = S.shape_sums_u8(u8)
    assert torch.equal(S.shape_sums_u8(u8), sums) and torch.equal(S.shape_sums_u8(u8[index].contiguous()), sums[index])


def test_output_buffers_are_honoured():
    from signature_gan_amd import shape as S
    x, w, t, *_ = batch_of(64, 5)
    want = S.shape_grad(dev(x), w, t)
    dx_out = torch.full((5, 1, 64, 64), 7.0, device=DEV)
    obj_out = torch.full((5,), 7.0, device=DEV)
    dx, obj, _ = S.shape_grad(dev(x), dev(w), dev(t), dx_out=dx_out, objective_out=obj_out)      # (device rows are taken too)
    assert dx is dx_out and obj is obj_out
    assert torch.equal(dx_out, want[0]) and torch.equal(obj_out, want[1])
    for bad in (dict(dx_out=torch.empty(5, 1, 64, 64, device=DEV, dtype=torch.float64)), dict(dx_out=torch.empty(4, 1, 64, 64, device=DEV)),
                dict(objective_out=torch.empty(6, device=DEV)), dict(objective_out=torch.empty(5))):
        with pytest.raises(ValueError):
            S.shape_grad(dev(x), w, t, **bad)
    for bad_w in (-w, w * np.nan):
        with pytest.raises(ValueError):
            S.shape_grad(dev(x), dev(bad_w), t)                                    # the device check


@functools.lru_cache(maxsize=None)
def generator_bytes():
    """(8, 64, 64) uint8 on the host: g_generate_u8 of latentcommon's 64x64 Generator at eight seeded latent vectors."""
    from signature_gan_amd.generator_vanilla_gan import Generator
    sd, z_star, z0 = projection_case()
    g = Generator(latent_dim=P_LATENT, output_size=P_SIZE).to(DEV)
    g.load_state_dict(sd)
    g.eval()
    z = torch.cat([z_star, z0, torch.randn(2, P_LATENT, generator=torch.Generator().manual_seed(3))]).to(DEV)
    return g._require_engine().g_generate_u8(z.contiguous()).cpu().numpy()


def byte_images(s):
    rng = np.random.default_rng(20 + s)
    sets = [rng.integers(0, 256, size=(5, s, s), dtype=np.uint8), np.zeros((1, s, s), np.uint8), np.full((1, s, s), 255, np.uint8),
            rng.integers(0, 256, size=(POOL, s, s), dtype=np.uint8)]
    if s == P_SIZE:
        sets.append(generator_bytes())
    return np.concatenate(sets)


@pytest.mark.parametrize("s", SC.SIZES)
def test_byte_sums_equal_the_integer_restatement(s):
    from signature_gan_amd import shape as S
    u8 = byte_images(s)
    got = S.shape_sums_u8(dev(u8))
    assert got.dtype == torch.int64 and got.shape == (len(u8), 6)
    assert np.array_equal(got.cpu().numpy(), S.reference_sums_u8(u8))
    assert np.array_equal(S.shape_sums_u8(dev(u8[:1]).unsqueeze(1)).cpu().numpy(), S.reference_sums_u8(u8[:1]))


@pytest.mark.parametrize("s", SC.SIZES)
def test_fp32_features_of_dequantised_bytes_agree_with_the_byte_side(s):
    """x = siggan_dequant_table[b] is b / 127.5 - 1 to fp32 rounding, so its ink differs from (255 - b) / 255 by a few 2^-24 per
    pixel, and every moment by that over the ink mass: the bound is 16 * 2^-24 / mass per image.  It is checked on the CPU
    between the two restatements first, and only the images it holds for are compared on the GPU (all-255 has no mass)."""
    from signature_gan_amd import _lib, shape as S
    u8 = byte_images(s)[:16] if s != P_SIZE else np.concatenate([byte_images(s)[:8], generator_bytes()])
    x = _lib.dequant_table()[u8]
    from_bytes = S.features_from_sums(S.reference_sums_u8(u8), s)
    with np.errstate(divide="ignore"):
        bound = 16.0 * 2.0 ** -24 / from_bytes[:, S.MASS]
    held = (from_bytes[:, S.MASS] > 0) & (np.abs(S.reference_features(x) - from_bytes).max(axis=1) <= bound)
    print(f"s = {s}: the bound holds on the CPU for {int(held.sum())} of {len(u8)} images")
    assert held.sum() >= len(u8) - 2
    got = S.shape_features(dev(x[held])).cpu().numpy()
    sums = S.shape_sums_u8(dev(u8[held])).cpu().numpy()
    err = np.abs(got - S.features_from_sums(sums, s)).max(axis=1)
    print(f"    worst error / bound on the GPU: {float((err / bound[held]).max()):.3f}")
    assert (err <= bound[held]).all()


def test_every_refusal_leaves_the_outputs_untouched():
    from signature_gan_amd import _lib
    lib = _lib.load()
    b, s = 2, 64
    x = torch.ones(b, 1, s, s, device=DEV)                                         # blank: every feature is 0
    u8 = torch.zeros(b, s, s, dtype=torch.uint8, device=DEV)                       # all ink
    w, t = torch.ones(b, 8, dtype=torch.float64, device=DEV), torch.zeros(b, 8, dtype=torch.float64, device=DEV)
    f = torch.full((b, 8), -7.0, dtype=torch.float64, device=DEV)
    dx = torch.full((b, 1, s, s), -7.0, device=DEV)
    o = torch.full((b,), -7.0, device=DEV)
    sums = torch.full((b, 6), -7, dtype=torch.int64, device=DEV)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr() if isinstance(v, torch.Tensor) else v)   # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = dict(x=x, b=b, s=s, w=w, t=t, f=f, dx=dx, o=o)
    bad = [dict(s=32), dict(s=100), dict(b=0), dict(b=-1), dict(x=None), dict(x=x.data_ptr() + 4), dict(dx=dx.data_ptr() + 8),
           dict(f=None, dx=None, o=None), dict(w=None), dict(t=None), dict(w=None, t=None, f=None), dict(w=None, t=None, dx=None)]
    for kw in bad:
        a = {**ok, **kw}
        rc = lib.siggan_shape_f32(0, p(a["x"]), a["b"], a["s"], p(a["w"]), p(a["t"]), p(a["f"]), p(a["dx"]), p(a["o"]), stream)
        assert rc == _lib.E_ARG, kw
    for args in ((None, b, s, sums), (u8.data_ptr() + 1, b, s, sums), (u8, 0, s, sums), (u8, b, 48, sums), (u8, b, s, None)):
        assert lib.siggan_shape_u8(0, p(args[0]), args[1], args[2], p(args[3]), stream) == _lib.E_ARG, args
    torch.cuda.synchronize()
    assert bool((f == -7.0).all()) and bool((dx == -7.0).all()) and bool((o == -7.0).all()) and bool((sums == -7).all())
    # and the same pointers with good arguments run
    assert lib.siggan_shape_f32(0, p(x), b, s, p(w), p(t), p(f), p(dx), p(o), stream) == 0
    assert lib.siggan_shape_u8(0, p(u8), b, s, p(sums), stream) == 0
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((sums[:, 0] == 255 * s * s).all())
