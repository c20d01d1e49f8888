"""The signature duplicator without a device: the binding against the header, the restatement (tests/warpcommon.py) on what
can be worked out by hand, the fold bound, the mistakes the GPU cases are meant to catch, the host-side plan under
sanitizers, every refusal's wording and the trainer's command line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import rngcommon as R
import warpcommon as W

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, warp
from signature_gan_amd import signature_verifier_train as ST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "signature-gan_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "siggan_warp.h")).read()


# ------------------------------------------------------------------------------------------------------ binding and header
def test_the_table_is_bound_and_exported():
    assert _lib._WARP_SIGNATURES in _lib.ADDED_GROUPS and "siggan_warp_u8" in _lib.ADDED_SYMBOLS
    assert "siggan_warp_u8" not in _lib.ALL_EXPORTS + _lib.EXTRA_SYMBOLS     # both are pinned whole by earlier tests
    assert "ADDED_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read(), "build() checks the library exports it"
    assert not [k for k in vars(_lib) if "WARP" in k and k.endswith("EXPORTS")]
    fn = getattr(C.CDLL(_lib.LIB_PATH), "siggan_warp_u8")            # the built library exports it
    assert fn is not None and _lib.load().siggan_warp_u8.argtypes == _lib._WARP_SIGNATURES["siggan_warp_u8"][1]
    proto = re.search(r"int siggan_warp_u8\((.*?)\);", HEADER, re.S).group(1)
    assert len(proto.split(",")) == len(_lib._WARP_SIGNATURES["siggan_warp_u8"][1]) == 15


def test_the_constants_agree_with_the_header():
    define = lambda name: re.search(rf"#define {name}\S* (\S+)", HEADER).group(1)
    assert int(define("SIGGAN_WARP_STREAM").rstrip("u"), 16) == W.SID_WARP == _lib.WARP_STREAM
    assert int(define("SIGGAN_WARP_MAX_SIZE")) == _lib.WARP_MAX_SIZE and int(define("SIGGAN_WARP_PARAMS")) == _lib.WARP_PARAMS
    assert int(define("SIGGAN_WARP_MAX_CTRL")) == W.MAX_CTRL == _lib.WARP_MAX_CTRL
    assert W.CELLS == _lib.WARP_CELLS == warp.CELLS
    others = [R.SID_Z, R.SID_ZG, R.SID_RANDN, R.SID_FC1, R.SID_FC2, R.SID_CLS] + [R.SID_DROP0 + l for l in range(0, 17)]
    assert W.SID_WARP not in others, "the warp's stream id is its own"
    for c in W.CELLS:
        assert warp.max_amplitude(c) == W.max_amp(c) == c * 512 // 5
    assert [W.max_amp(c) for c in W.CELLS] == [819, 1638, 3276]
    assert warp.control_grid_shape(40, 68, 16) == W.grid(40, 68, 16) == (6, 8)
    assert warp.control_grid_shape(8, 8, 8) == (4, 4) and warp.control_grid_shape(128, 128, 8) == (19, 19)


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("c", W.CELLS)
def test_the_weights_sum_to_six_c_cubed(c):
    b = W.weights(np.arange(c), c)
    assert (b >= 0).all() and (b.sum(0) == 6 * c ** 3).all()
    assert list(b[:, 0]) == [c ** 3, 4 * c ** 3, c ** 3, 0], "at a control point: 1/6, 4/6, 1/6, 0"


@pytest.mark.parametrize("c", W.CELLS)
def test_a_constant_grid_is_a_constant_field_and_the_rounding_is_half_up(c):
    gy, gx = W.grid(24, 36, c)
    for v in (0, 1, -1, 77, -W.max_amp(c), W.MAX_CTRL, -W.MAX_CTRL):
        assert (W.displacement(np.full((2, gy, gx), v), 24, 36, c) == v).all()
    assert (W.displacement(np.full((2, gy, gx), 3 * W.MAX_CTRL), 24, 36, c) == W.MAX_CTRL).all(), "control values are clamped"
    # one control point of 3 at a grid node reaches the pixel on it with weight 16/36: 4/3 -> 1; a point of -3: -4/3 -> -1;
    # a point of 9 at the diagonal neighbour's weight 1/36: 1/4 -> 0; 18: 1/2 -> 1 (half up); -18: -1/2 -> 0 (half up)
    for v, centre, corner in ((3, 1, 0), (-3, -1, 0), (9, 4, 0), (18, 8, 1), (-18, -8, 0)):
        D = np.zeros((2, gy, gx), np.int64)
        D[:, 2, 2] = v                                              # control point (2, 2) sits at pixel (c, c)
        d = W.displacement(D, 24, 36, c)
        if c < 24:
            assert d[0, c, c] == centre and d[1, c, c] == centre
        assert d[0, 0, 0] == corner, (v, d[0, 0, 0])               # pixel (0, 0) sees point (2, 2) with weight 1/36


@pytest.mark.parametrize("c", W.CELLS)
def test_the_displacement_stays_within_the_amplitude(c):
    h, w = 40, 68
    gy, gx = W.grid(h, w, c)
    for seed, draw_id in W.DRAWS:
        for amp in ((W.max_amp(c), W.max_amp(c)), (1, 0), (5, 300)):
            D = W.control_points(seed, draw_id, amp, h, w, c)
            assert D.shape == (2, gy, gx) and (np.abs(D[0]) <= amp[0]).all() and (np.abs(D[1]) <= amp[1]).all()
            d = W.displacement(D, h, w, c)
            assert (np.abs(d[0]) <= amp[0]).all() and (np.abs(d[1]) <= amp[1]).all()
    assert (W.control_points(3, 4, (10 ** 6, -5), h, w, c)[1] == 0).all(), "an amplitude outside the range is clamped into it"
    assert np.abs(W.control_points(3, 4, (10 ** 6, -5), h, w, c)[0]).max() <= W.max_amp(c)


def test_zero_amplitude_and_the_identity_are_a_copy():
    for img in W.contents(40, 68, seed=3):
        for c in W.CELLS:
            for fill in (0, 255):
                out, disp = W.warp_one(img, 9, 11, (0, 0), W.IDENTITY, c, fill)
                assert np.array_equal(out, img) and not disp.any()


def test_the_sample_by_hand():
    img = np.array([[0, 100, 200, 40]] * 2, np.uint8)
    pos = np.zeros((2, 2, 4), np.int64)
    pos[0] = [[128, 256 + 64, -128, 3 * 256 + 128]] * 2             # x: between 0|1, a quarter past 1, half outside left, half outside right
    out = W.sample(img, pos, 255)
    assert list(out[0]) == [50, 125, (255 * 128 * 256 + 0 + 32768) >> 16, (40 * 128 * 256 + 255 * 128 * 256 + 32768) >> 16]
    pos[1] = 256 + 128                                              # y: half below the last row -> half fill
    assert W.sample(img, pos, 0)[0, 0] == (128 * 128 * 100 + 32768) >> 16 == 25


def test_the_base_map_does_not_wrap():
    a = (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31, -2 ** 31)
    b = W.base_map(a, 128, 128)
    assert b[0, 127, 127] == ((2 ** 31 - 1) * 255) >> 8 and b[1, 127, 127] == (-2 ** 31 * 255) >> 8
    img = W.contents(8, 8)[4]
    assert (W.warp_one(img, 1, 1, (0, 0), a, 8, 7)[0][1:, 1:] == 7).all(), "far outside: the fill"


@pytest.mark.parametrize("c", W.CELLS)
def test_the_map_does_not_fold_at_the_largest_amplitude(c):
    """At amp = floor(0.4 c 256) the source position strictly increases along every row and column, for the worst-case
    patterns and for 50 seeded random grids; at 0.7 cells the half-plane step folds."""
    h = w = 64
    gy, gx = W.grid(h, w, c)
    amp = W.max_amp(c)
    for p in W.fold_patterns(gy, gx, amp):
        assert W.min_advance(p, h, w, c) > 0
    rng = np.random.default_rng(1000 + c)
    for _ in range(50):
        assert W.min_advance(rng.integers(-amp, amp + 1, (2, gy, gx)), h, w, c) > 0
    for k in range(3):                                               # the restatement's own draws
        assert W.min_advance(W.control_points(5, k, (amp, amp), h, w, c), h, w, c) > 0
    step = W.fold_patterns(gy, gx, int(0.7 * c * 256))[3]
    assert step.max() <= W.MAX_CTRL and W.min_advance(step, h, w, c) < 0


# -------------------------------------------------------------------------- the cases tell a mistaken generator from the right one
@pytest.mark.parametrize("h,w,c", W.SHAPES[:4])
def test_the_cases_catch_each_mistake(h, w, c):
    img = W.contents(h, w, seed=1)[4]
    amp = (W.max_amp(c), W.max_amp(c) // 2)
    for seed, draw_id in W.DRAWS:
        right, field = W.warp_one(img, seed, draw_id, amp, W.IDENTITY, c, 255)
        for mut in (dict(sid=W.SID_WARP + 1), dict(sid=R.SID_RANDN), dict(mutant="id_as_index"), dict(mutant="swap"), dict(mutant="low_half")):
            wrong, wrong_field = W.warp_one(img, seed, draw_id, amp, W.IDENTITY, c, 255, **mut)
            assert not np.array_equal(field, wrong_field), mut
            assert not np.array_equal(right, wrong), mut
    # draw ids 2^32 - 1 and 2^32 differ, and a draw id's high word is not dropped
    a = W.control_points(9, (1 << 32) - 1, amp, h, w, c)
    b = W.control_points(9, 1 << 32, amp, h, w, c)
    assert not np.array_equal(a, b) and not np.array_equal(b, W.control_points(9, 0, amp, h, w, c))
    assert ((1 << 32) - 1 in [d for _, d in W.DRAWS]) and (1 << 32 in [d for _, d in W.DRAWS]) and any(s >> 32 for s, _ in W.DRAWS)


# ------------------------------------------------------------------------------------------------------------ the host plan
def test_the_plan_header_under_sanitizers(tmp_path):
    """csrc/warp_plan.h -- grid extents, the LDS layout, the amplitude bound, the weights and the rounding -- by the
    stand-alone csrc/warp_plan_check.cpp under AddressSanitizer and UBSan: this is what the test is about, so it starts the
    compiler and the program."""
    exe = str(tmp_path / "warp_plan_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "warp_plan_check.cpp")],
                   check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.fullmatch(r"OK \d+", run.stdout.strip()) and int(run.stdout.split()[1]) > 3 * (200000 + 128 * 32), run.stdout + run.stderr


# --------------------------------------------------------------------------------------------------------- the host helpers
def test_param_rows_and_the_affine():
    ids = np.array([0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1], np.uint64)
    aff = np.arange(24).reshape(4, 6)
    rows = warp.param_rows(ids, (7, 9), aff)
    assert rows.dtype == np.int32 and rows.shape == (4, 12)
    assert [tuple(r) for r in rows[:, :2].view(np.uint32)] == [(0, 0), (0xFFFFFFFF, 0), (0, 1), (0xFFFFFFFF, 0xFFFFFFFF)]
    assert (rows[:, 2] == 7).all() and (rows[:, 3] == 9).all() and np.array_equal(rows[:, 4:10], aff) and not rows[:, 10:].any()
    spec = warp.WarpSpec()
    a, draws = warp.draw_affine(spec, 3, 5, (40, 68))
    assert a.dtype == np.int32 and [tuple(r) for r in a] == [W.IDENTITY] * 3 and (draws["scale"] == 1).all()
    assert tuple(warp.affine_fixed(5.0, 0.1, 0.9, 0.0, 0.0, 40, 68)[0]) == W.tilted_affine(40, 68)
    # a pure shift of (+3, -2): the source is read 3 to the left and 2 below
    assert tuple(warp.affine_fixed(0, 0, 1, 3, -2, 8, 8)[0]) == (65536, 0, -3 * 65536, 0, 65536, 2 * 65536)
    spec = warp.WarpSpec(rotate_deg=5, slant=0.1, scale=0.1, shift_px=2)
    a, draws = warp.draw_affine(spec, 4, 5, (64, 64), draw_ids=[10, 11, 12, 13])
    b, _ = warp.draw_affine(spec, 2, 5, (64, 64), draw_ids=[12, 10])
    assert np.array_equal(a[[2, 0]], b), "an image's affine depends on the seed and its draw id alone"
    assert len({tuple(r) for r in a}) == 4 and not np.array_equal(a, warp.draw_affine(spec, 4, 6, (64, 64), draw_ids=[10, 11, 12, 13])[0])
    assert (np.abs(draws["rotate_deg"]) <= 5).all() and (np.abs(draws["scale"] - 1) <= 0.1).all() and (np.abs(draws["shift_x"]) <= 2).all()


# ------------------------------------------------------------------------------------------------------------- the refusals
def refused(text, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value) == text


def test_the_spec_refusals_word_for_word():
    S = warp.WarpSpec
    refused("cell must be an integer, got 16.0", S(cell=16.0).check)
    refused("cell must be one of (8, 16, 32), got 12", S(cell=12).check)
    refused("amplitude must be one number or (ax, ay), got (1, 2, 3)", S(amplitude=(1, 2, 3)).check)
    refused("amplitude x must be a finite number, got 'a'", S(amplitude=("a", 1)).check)
    refused("amplitude y must be a finite number, got nan", S(amplitude=(1, float("nan"))).check)
    refused("amplitude x = 1639 / 256 px outside [0, 1638 / 256] (0.4 cells of 16 px)", S(amplitude=(1639 / 256, 0)).check)
    refused("amplitude y = -1 / 256 px outside [0, 819 / 256] (0.4 cells of 8 px)", S(cell=8, amplitude=(0, -1 / 256)).check)
    refused("amplitude x = 3277 / 256 px outside [0, 3276 / 256] (0.4 cells of 32 px)", S(cell=32, amplitude=3277 / 256).check)
    S(cell=32, amplitude=3276 / 256).check(), S(cell=8, amplitude=(819 / 256, 0)).check(), S(amplitude=1638 / 256).check()
    refused("rotate_deg = -1 < 0", S(rotate_deg=-1).check)
    refused("rotate_deg = 46 outside [0, 45]", S(rotate_deg=46).check)
    refused("slant = 1.5 outside [0, 1]", S(slant=1.5).check)
    refused("scale = 0.6 outside [0, 0.5]", S(scale=0.6).check)
    refused("shift_px = 129 outside [0, 128]", S(shift_px=129).check)
    refused("shift_px must be a finite number, got None", S(shift_px=None).check)
    refused("fill must be an integer, got 1.5", S(fill=1.5).check)
    refused("fill = 256 outside [0, 255]", S(fill=256).check)
    refused("cell must be one of (8, 16, 32), got 4", warp.max_amplitude, 4)
    refused("cell must be one of (8, 16, 32), got 64", warp.control_grid_shape, 8, 8, 64)
    refused("h and w must be positive, got 0 and 8", warp.control_grid_shape, 0, 8, 8)


def test_the_call_refusals_word_for_word():
    """In _call's order: type, dtype, rank, sizes; then the spec, seed, index, draw ids, affine; then the device."""
    spec = warp.WarpSpec()
    u8 = torch.zeros((2, 8, 8), dtype=torch.uint8)
    refused("images must be a tensor, got ndarray", warp.warp_u8, np.zeros((1, 8, 8), np.uint8), spec, 0)
    refused("images must be torch.uint8, got torch.float32", warp.warp_u8, torch.zeros(1, 8, 8), spec, 0)
    refused("images must be (N, H, W) or (N, 1, H, W), got (8, 8)", warp.warp_u8, u8[0], spec, 0)
    refused("images holds no image", warp.warp_u8, u8[:0], spec, 0)
    refused("height = 129 outside [1, 128]", warp.warp_u8, torch.zeros((1, 129, 8), dtype=torch.uint8), spec, 0)
    refused("width = 6 must be a multiple of 4 in [4, 128]", warp.warp_u8, torch.zeros((1, 8, 6), dtype=torch.uint8), spec, 0)
    refused("width = 132 must be a multiple of 4 in [4, 128]", warp.warp_u8, torch.zeros((1, 8, 132), dtype=torch.uint8), spec, 0)
    refused("spec must be a WarpSpec, got dict", warp.warp_u8, u8, {}, 0)
    refused("cell must be one of (8, 16, 32), got 7", warp.warp_u8, u8, warp.WarpSpec(cell=7), 0)
    refused("amplitude x = 1639 / 256 px outside [0, 1638 / 256] (0.4 cells of 16 px)", warp.warp_u8, u8, warp.WarpSpec(amplitude=1639 / 256), 0)
    refused("seed must be an integer, got 1.0", warp.warp_u8, u8, spec, 1.0)
    refused("seed = -1 outside [0, 2^64)", warp.warp_u8, u8, spec, -1)
    refused(f"seed = {1 << 64} outside [0, 2^64)", warp.warp_u8, u8, spec, 1 << 64)
    refused("index must be a non-empty 1-D integer array, got float64 (2,)", warp.warp_u8, u8, spec, 0, index=[0.0, 1.0])
    refused("index must be a non-empty 1-D integer array, got int64 (0,)", warp.warp_u8, u8, spec, 0, index=np.zeros(0, np.int64))
    refused("draw_ids holds 3 values for 2 images", warp.warp_u8, u8, spec, 0, draw_ids=[1, 2, 3])
    refused("draw_ids holds 2 values for 3 images", warp.warp_u8, u8, spec, 0, draw_ids=[1, 2], index=[0, 0, 1])
    refused("draw id = -1 outside [0, 2^64)", warp.warp_u8, u8, spec, 0, draw_ids=[0, -1])
    refused("affine must be (2, 6) integers that fit int32, got int64 (1, 6)", warp.warp_u8, u8, spec, 0, affine=np.zeros((1, 6), np.int64))
    refused("affine must be (2, 6) integers that fit int32, got float64 (2, 6)", warp.warp_u8, u8, spec, 0, affine=np.zeros((2, 6)))
    refused("affine must be (2, 6) integers that fit int32, got int64 (2, 6)", warp.warp_u8, u8, spec, 0, affine=np.full((2, 6), 1 << 31))
    refused("images must live on a ROCm device ('cuda:N'); there is no CPU path", warp.warp_u8, u8, spec, 0)
    refused("copies must be an integer, got 2.0", warp.duplicate_u8, u8, 2.0, spec, 0)
    refused("copies = 0 < 1", warp.duplicate_u8, u8, 0, spec, 0)
    refused("first_id = -1 outside [0, 2^64)", warp.duplicate_u8, u8, 1, spec, 0, first_id=-1)
    refused(f"first_id = {(1 << 64) - 1}: the draw ids of 2 copies leave [0, 2^64)", warp.duplicate_u8, u8, 1, spec, 0, first_id=(1 << 64) - 1)


def test_the_library_refuses_without_a_device():
    """The C side's own refusals come before any device call, so they can be read here: nothing is launched."""
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    a = C.addressof(buf)
    src, prm, out = a, a + 1024, a + 2048

    def call(src=src, n_src=1, prm=prm, ctrl=None, out=out, field=None, n=1, h=8, w=8, cell=8, fill=255):
        rc = lib.siggan_warp_u8(0, src, n_src, None, prm, ctrl, out, field, n, h, w, cell, fill, 0, None)
        return rc, lib.siggan_last_error().decode()

    assert call(src=None) == (-1, "siggan_warp_u8: null tensor") and call(prm=None)[0] == -1 and call(out=None)[0] == -1
    assert call(n=0) == (-1, "siggan_warp_u8: n must be in 1..2^20, got 0") and call(n=(1 << 20) + 1)[0] == -1
    assert call(n_src=0) == (-1, "siggan_warp_u8: no source image")
    assert call(h=0) == (-1, "siggan_warp_u8: h must be in 1..128, got 0") and call(h=129)[0] == -1
    assert call(w=6) == (-1, "siggan_warp_u8: w must be a multiple of 4 in 4..128, got 6") and call(w=132)[0] == -1 and call(w=0)[0] == -1
    assert call(cell=4) == (-1, "siggan_warp_u8: cell must be 8, 16 or 32, got 4") and call(cell=64)[0] == -1
    assert call(fill=256) == (-1, "siggan_warp_u8: fill must be a byte value") and call(fill=-1)[0] == -1
    assert call(src=a + 2)[1].endswith("must be 4-byte aligned") and call(field=a + 3074)[0] == -1
    assert call(ctrl=a + 3073) == (-1, "siggan_warp_u8: ctrl_dev must be 2-byte aligned")
    assert call(out=a + 60) == (-1, "siggan_warp_u8: out_dev overlaps src_dev")         # out begins inside the one source image
    assert call(out=a, src=a + 60)[0] == -1 and call(out=a + 64, n_src=2)[0] == -1 and call(src=a + 64, out=a, n=2)[0] == -1


# ------------------------------------------------------------------------------------------------------- the trainer's flags
def test_the_trainer_refuses_elastic_with_the_host_pipeline(tmp_path, capsys, monkeypatch):
    assert ST.check_elastic("host", None) is None and ST.check_elastic("device", None) is None
    assert ST.check_elastic("device", 2.5, 8) == warp.WarpSpec(cell=8, amplitude=(2.5, 2.5))
    assert ST.check_elastic("device", 3) == warp.WarpSpec(cell=16, amplitude=(3, 3))
    with pytest.raises(ValueError, match="elastic_cell needs elastic"):
        ST.check_elastic("device", None, 8)
    with pytest.raises(ValueError, match="outside"):
        ST.check_elastic("device", 7.0)
    with pytest.raises(ValueError, match="the elastic warp needs --input_pipeline device"):
        ST.train_model(str(tmp_path), None, 1, str(tmp_path / "models"), elastic=2.0)
    with pytest.raises(ValueError, match="the elastic warp needs --input_pipeline device"):
        ST.main(["--data_dir", str(tmp_path), "--model_output", str(tmp_path / "models"), "--elastic", "2"])
    assert not (tmp_path / "models").exists()                         # refused before anything is done
    seen = {}
    monkeypatch.setattr(ST, "train_model", lambda **kw: seen.update(kw) or {})
    ST.main(["--data_dir", "d", "--input_pipeline", "device", "--elastic", "1.5", "--elastic_cell", "8"])
    assert seen["elastic"] == 1.5 and seen["elastic_cell"] == 8
    seen.clear()
    ST.main(["--data_dir", "d"])
    assert "elastic" not in seen and "elastic_cell" not in seen         # an old command line: the old call
    capsys.readouterr()
