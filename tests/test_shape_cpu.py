"""CPU-only checks of the shape attributes: the numpy fp64 restatement (shape.reference_features / reference_grad) on its own
-- its gradient against central differences, the shear law of the slant, its sensitivity to the order of the sums --, the
byte side's host expression (features_from_sums) and its integer bounds, the ctypes table against include/siggan_shape.h and
every refusal of the two C calls (argument checks in front of any HIP call, so they run without a GPU), the binding's own
refusals, edit_latents' target and weight construction and refusals, calculate_shape_attributes' summary, and the CLI flags."""
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import shapecommon as SC
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import shape as S


@pytest.mark.parametrize("s", SC.SIZES)
def test_reference_grad_is_the_central_difference_of_the_reference_objective(s):
    """On three regular images (two smooth ones and the slanted bar), at the four corners and 256 seeded pixels each, in fp64,
    to 1e-7 of the image's largest |dx|.  The objective is a smooth function of one pixel; with h = 1e-4 the truncation error
    is far below the bound.  Measured when the test was written: 2.3e-9 (s = 64), 7.7e-9 (s = 128)."""
    x = SC.regular_images(3, s).astype(np.float64)
    f = S.reference_features(x)
    w, t = SC.objective_rows(3, f)
    dx, obj, feats = S.reference_grad(x, w, t)
    assert np.array_equal(feats, f) and np.array_equal(obj, S.reference_objective(f, w, t))
    rng = np.random.default_rng(3 + s)
    h, worst = 1e-4, 0.0
    for i in range(3):
        pixels = [(0, 0), (0, s - 1), (s - 1, 0), (s - 1, s - 1)] + [tuple(p) for p in rng.integers(0, s, size=(256, 2))]
        for r, c in pixels:
            side = []
            for step in (h, -h):
                y = x[i:i + 1].copy()
                y[0, r, c] += step
                side.append(S.reference_objective(S.reference_features(y), w[i:i + 1], t[i:i + 1])[0])
            worst = max(worst, abs((side[0] - side[1]) / (2 * h) - dx[i, r, c]) / np.abs(dx[i]).max())
    print(f"s = {s}: worst |central difference - reference_grad| / max |dx| = {worst:.2e}")
    assert worst <= 1e-7


@pytest.mark.parametrize("s", SC.SIZES)
def test_shearing_by_whole_pixels_per_row_adds_the_shear_to_the_slant(s):
    """Row r of a blob is moved right by m (r - r0) pixels.  Because one row is 1 / s in v and one pixel 1 / s in u, every ink
    pixel centre moves by exactly m (v - v0) in u onto another pixel centre: the shear x' = x + m y holds without any
    discretisation error as long as no ink leaves the frame, so du' = du + m dv, sxy' = sxy + m syy and slant' = slant + m up
    to fp64 rounding -- about s^2 * 2^-53 / syy, below 1e-10 here.  m > 0 leans to the left ("\\"), m < 0 to the right ("/")."""
    rng = np.random.default_rng(5 + s)
    x = np.ones((s, s))
    rows, cols = slice(s // 2 - s // 8, s // 2 + s // 8), slice(s // 2 - s // 8, s // 2 + s // 8)
    x[rows, cols] = 1.0 - 2.0 * rng.uniform(0.2, 1.0, size=(s // 4, s // 4))
    base = S.reference_features(x[None])[0]
    assert base[S.SYY] >= 1e-3
    for m in (-2, -1, 1, 2):
        y = np.ones((s, s))
        for r in range(rows.start, rows.stop):
            y[r] = np.roll(x[r], m * (r - s // 2))
        f = S.reference_features(y[None])[0]
        assert abs(f[S.SLANT] - (base[S.SLANT] + m)) <= 1e-10, (m, f[S.SLANT], base[S.SLANT])
        assert abs(f[S.MASS] - base[S.MASS]) <= 1e-15 and abs(f[S.SYY] - base[S.SYY]) <= 1e-15
    bar = S.reference_features(SC.slanted_bar(s, k=-0.5)[None])[0]
    assert -0.6 < bar[S.SLANT] < -0.4                                              # "/" is negative


@pytest.mark.parametrize("s", SC.SIZES)
def test_reversing_the_summation_order_moves_the_features_by_less_than_1e_11(s):
    """The evidence for the GPU test's 1e-9: another order of the same fp64 sums."""
    x = SC.regular_images(6, s)
    d = np.abs(S.reference_features(x) - S.reference_features(x, reverse=True)).max()
    print(f"s = {s}: features forward vs reversed sums: {d:.2e}")
    assert d <= 1e-11


@pytest.mark.parametrize("s", SC.SIZES)
def test_features_from_sums_is_the_restatement_on_byte_ink(s):
    rng = np.random.default_rng(9 + s)
    u8 = np.concatenate([rng.integers(0, 256, size=(3, s, s), dtype=np.uint8),
                         np.full((1, s, s), 255, np.uint8), np.zeros((1, s, s), np.uint8),
                         ((SC.regular_images(3, s) + 1) * 127.5).clip(0, 255).astype(np.uint8)])
    got = S.features_from_sums(S.reference_sums_u8(u8), s)
    ink = (255.0 - u8.astype(np.float64)) / 255.0
    want = S.reference_features(1.0 - 2.0 * ink)
    assert np.abs(got - want).max() <= 1e-13
    assert np.all(got[3, 1:] == 0.0) and got[3, 0] == 0.0                          # all-255: empty
    assert got[4, 0] == 1.0 and got[4, S.CX] == 0.0 and got[4, S.CY] == 0.0        # all ink: centred
    with pytest.raises(ValueError):
        S.features_from_sums(np.zeros((1, 6), np.int32), s)
    with pytest.raises(ValueError):
        S.features_from_sums(np.zeros((1, 6), np.int64), 32)


def test_integer_bounds_of_the_byte_sums():
    """All ink at s = 128 maximises the even sums; ink on one half (p > 0, q > 0) the odd ones: every sum stays below 6.8e10, a
    lane's 64 terms below 2^31, and the products features_from_sums forms below 2.9e17 (int64 holds 9.2e18)."""
    s = 128
    full = S.reference_sums_u8(np.zeros((1, s, s), np.uint8))[0]
    half = np.full((1, s, s), 255, np.uint8)
    half[0, s // 2:, s // 2:] = 0
    quarter = S.reference_sums_u8(half)[0]
    assert full[0] == 255 * s * s and full[1] == full[2] == full[5] == 0
    assert max(int(np.abs(full).max()), int(np.abs(quarter).max())) < 6.8e10
    assert 64 * 255 * 127 * 127 < 2 ** 31
    for m in (full, quarter):
        s0, sp, sq, spp, sqq, spq = (int(v) for v in m)
        assert max(abs(s0 * spp - sp * sp), abs(s0 * sqq - sq * sq), abs(s0 * spq - sp * sq), s0 * spp, s0 * sqq, sp * sp) < 2.9e17


def test_library_exports_the_shape_header():
    with open(os.path.join(ROOT, "include", "siggan_shape.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\bint\s+(siggan_\w+)\s*\(", header))
    assert declared == set(_lib.SHAPE_EXPORTS) == {"siggan_shape_f32", "siggan_shape_u8"}
    assert not set(_lib.SHAPE_EXPORTS) & set(_lib.EXPORTS)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in siggan_shape.h but not exported"
    assert lib.siggan_abi_version() == 4                                           # symbols only added
    assert int(re.search(r"#define SIGGAN_SHAPE_FEATURES\s+(\d+)", header).group(1)) == _lib.SHAPE_FEATURES == len(S.FEATURES)
    assert int(re.search(r"#define SIGGAN_SHAPE_SUMS\s+(\d+)", header).group(1)) == _lib.SHAPE_SUMS
    assert float(re.search(r"#define SIGGAN_SHAPE_SYY_MIN\s+(\S+)", header).group(1)) == _lib.SHAPE_SYY_MIN
    for k, name in enumerate(S.FEATURES):
        assert int(re.search(rf"#define SIGGAN_SHAPE_{name.upper()}\s+(\d+)", header).group(1)) == k
    assert "negative slant" in header.lower().replace("\n * ", " ")


def refusals_f32(x=0x1000, b=1, s=64, w=0x2000, t=0x3000, f=0x4000, dx=0x5000, o=0x6000):
    return _lib.load().siggan_shape_f32(0, x, b, s, w, t, f, dx, o, None)


def test_every_refusal_of_the_c_calls_comes_before_any_hip_call():
    """The pointers are made-up addresses: a call that got past its argument checks would touch HIP (and fail differently)."""
    lib = _lib.load()
    bad = [dict(s=32), dict(s=96), dict(s=256), dict(b=0), dict(b=-3), dict(x=None), dict(x=0x1004), dict(dx=0x5008),
           dict(f=None, dx=None, o=None), dict(w=None), dict(t=None), dict(w=None, t=None, dx=None), dict(w=None, t=None, f=None, o=None),
           dict(f=0x4004), dict(w=0x2004), dict(t=0x3004)]
    for kw in bad:
        assert refusals_f32(**kw) == _lib.E_ARG, kw
        assert lib.siggan_last_error()
    for args in ((None, 1, 64, 0x2000), (0x1002, 1, 64, 0x2000), (0x1000, 0, 64, 0x2000), (0x1000, 1, 100, 0x2000), (0x1000, 1, 64, None),
                 (0x1000, 1, 64, 0x2004)):
        assert lib.siggan_shape_u8(0, *args, None) == _lib.E_ARG, args


def test_binding_refusals_need_no_device():
    x = torch.zeros(2, 1, 64, 64)
    for bad in (x.numpy(), x.double(), torch.zeros(2, 64, 32), torch.zeros(2, 2, 64, 64), torch.zeros(2, 32, 32), torch.zeros(0, 64, 64), x):
        with pytest.raises(ValueError):
            S.shape_features(bad)                                                  # (the last one: not on a ROCm device)
    with pytest.raises(ValueError):
        S.shape_sums_u8(torch.zeros(2, 64, 64))
    with pytest.raises(ValueError):
        S.shape_sums_u8(torch.zeros(2, 64, 64, dtype=torch.uint8))                 # a CPU tensor
    dev = torch.device("cpu")
    ok = np.ones((2, 8))
    assert S._check_rows("weights", ok, 2, dev, True).dtype == torch.float64
    for bad in (-ok, ok * np.nan, ok * np.inf, np.ones((2, 7)), np.ones((3, 8))):
        with pytest.raises(ValueError):
            S._check_rows("weights", bad, 2, dev, True)
    with pytest.raises(ValueError):
        S._check_rows("targets", torch.ones(2, 8), 2, dev, False)                  # a float32 tensor
    S._check_rows("targets", ok * np.nan, 2, dev, False)                           # targets may be anything


def test_edit_targets_and_weights():
    from signature_gan_amd.utils.inference import edit_targets
    f0 = torch.tensor([[0.1, 0.02, -0.03, 0.05, 0.01, -0.002, -0.2, 0.06],
                       [1e-5, 0.0, 0.0, 1e-4, 1e-4, 0.0, 0.0, 2e-4]], dtype=torch.float64)
    w, t = edit_targets(f0, slant_delta=-0.25)
    assert torch.equal(w, torch.tensor([[0, 0, 0, 0, 0, 0, 1.0, 0]] * 2, dtype=torch.float64))
    assert torch.equal(t[:, S.SLANT], f0[:, S.SLANT] - 0.25) and torch.equal(t[:, :6], f0[:, :6]) and torch.equal(t[:, 7], f0[:, 7])
    w, t = edit_targets(f0, size_scale=1.5, boldness_scale=0.8, shift=(0.1, 0.0), shape_weight=3.0)
    assert torch.equal(t[:, S.SPREAD], f0[:, S.SPREAD] * 2.25) and torch.equal(t[:, S.MASS], f0[:, S.MASS] * 0.8)
    assert torch.equal(t[:, S.CX], f0[:, S.CX] + 0.1) and torch.equal(t[:, S.CY], f0[:, S.CY])
    assert torch.equal(t[:, 3:7], f0[:, 3:7])                                      # sxx, syy, sxy (and the slant) get no target
    assert torch.equal(w[:, 3:7], torch.zeros(2, 4, dtype=torch.float64))
    assert w[0, S.MASS] == 3.0 / (0.1 * 0.1) and w[0, S.SPREAD] == 3.0 / (0.06 * 0.06)   # relative residuals
    assert w[1, S.MASS] == 3.0 / 1e-6 and w[1, S.SPREAD] == 3.0 / 1e-6             # the floor of the scale
    assert w[0, S.CX] == w[0, S.CY] == 3.0                                         # a shift holds both coordinates
    assert bool((w >= 0).all()) and bool(torch.isfinite(w).all())
    with pytest.raises(ValueError):
        edit_targets(f0.float())


def test_edit_refusals_are_host_code():
    from signature_gan_amd.utils.inference import check_edit, edit_latents
    assert check_edit(slant_delta=0.1) == (0.1, 1.0, 1.0, (0.0, 0.0))
    assert check_edit(shift=[0, 0.2])[3] == (0.0, 0.2)
    for kw in (dict(), dict(slant_delta=0.0, size_scale=1.0), dict(slant_delta=float("nan")), dict(size_scale=0.0),
               dict(boldness_scale=-1.0), dict(shift=(0.1,)), dict(shift=0.1), dict(shift=(0.1, float("inf"))),
               dict(slant_delta=0.1, steps=0), dict(slant_delta=0.1, lr=0.0), dict(slant_delta=0.1, keep_weight=-1.0),
               dict(slant_delta=0.1, shape_weight=0.0), dict(slant_delta=0.1, prior_weight=float("nan")),
               dict(slant_delta=0.1, realism_weight=1.0)):
        with pytest.raises(ValueError):
            check_edit(**kw)
    check_edit(slant_delta=0.1, realism_weight=1.0, has_discriminator=True)
    with pytest.raises(ValueError, match="no edit"):
        edit_latents(None, torch.zeros(1, 100))                                    # refused before the Generator is looked at


def test_shape_attributes_summary():
    from signature_gan_amd.utils.metrics import shape_attributes_from_features
    f = np.zeros((4, 8))
    f[:3, 0] = (0.1, 0.2, 0.3)
    f[:3, S.SLANT] = (-0.5, 0.0, 0.1)
    d = shape_attributes_from_features(f)
    assert d["images"] == 4 and d["empty"] == 1 and set(d) == {"images", "empty", *S.FEATURES}
    assert set(d["slant"]) == {"mean", "std", "p5", "p50", "p95"}
    assert d["slant"]["p50"] == 0.0 and abs(d["slant"]["mean"] + 0.4 / 3) < 1e-15   # over the three images with ink
    assert abs(d["mass"]["mean"] - 0.15) < 1e-15                                    # over all four
    assert shape_attributes_from_features(np.zeros((2, 8)))["slant"] is None
    with pytest.raises(ValueError):
        shape_attributes_from_features(np.zeros((0, 8)))


def test_cli_flags():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import generate_signatures as gs
    plain = gs.parse_args(["--checkpoint", "c.pt"])
    assert not any(k.startswith("edit") for k in vars(plain))                      # the namespace of a plain run is what it was
    a = gs.parse_args(["--checkpoint", "c.pt", "--edit", "--edit_slant_delta", "-0.2", "--edit_shift", "0.1", "0", "--edit_steps", "5"])
    kw = gs.edit_kwargs(a)
    assert kw == dict(slant_delta=-0.2, size_scale=1.0, boldness_scale=1.0, shift=(0.1, 0.0), steps=5, lr=0.02, keep_weight=1.0,
                      realism_weight=0.0)
    for bad in (["--edit"], ["--edit_slant_delta", "0.1"], ["--edit", "--edit_size_scale", "0"], ["--edit", "--edit_slant_delta", "0.1", "--edit_steps", "0"],
                ["--edit", "--edit_slant_delta", "0.1", "--filter_by_realism"], ["--edit", "--edit_slant_delta", "0.1", "--pen_width", "3"],
                ["--edit", "--edit_slant_delta", "0.1", "--despeckle"], ["--edit", "--edit_slant_delta", "0.1", "--morph"]):
        with pytest.raises(SystemExit):
            gs.parse_args(["--checkpoint", "c.pt"] + bad)
    e = ev.parse_args(["--checkpoint", "c.pt"])
    assert e.shape is False and "shape" not in vars(e)
    assert ev.parse_args(["--checkpoint", "c.pt", "--shape"]).shape is True
