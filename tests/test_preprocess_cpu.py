"""Scan preprocessing without a device: the binding against the header, the registry, the restatement
(tests/preprocesscommon.py) on inputs small enough to work out by hand, the host-side geometry under sanitizers, every
refusal's wording and the command lines."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preprocesscommon as PC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, preprocess, preprocess_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "signature-gan_amd", "csrc")


# ---------------------------------------------------------------------------------------------------- binding, registry
def test_the_binding_is_the_header():
    header = open(os.path.join(ROOT, "include", "siggan_preprocess.h")).read()
    declared = re.findall(r"^(?:int|size_t) (siggan_\w+)\(", header, flags=re.M)
    assert tuple(declared) == tuple(_lib._PREPROCESS_SIGNATURES) == ("siggan_preprocess_workspace", "siggan_preprocess_u8")
    columns = re.findall(r"^\s+SIGGAN_PP_([A-Z0-9_]+),?\s", header[header.index("columns of stats_dev"):], flags=re.M)
    assert columns[-1] == "COUNT" and tuple(c.lower() for c in columns[:-1]) == preprocess.STAT_NAMES
    assert len(columns) - 1 == _lib.PP_COUNT == PC.COUNT == 13
    for i, name in enumerate(preprocess.STAT_NAMES):
        assert getattr(preprocess, name.upper()) == getattr(PC, name.upper()) == i
    limits = dict(re.findall(r"#define SIGGAN_PP_(\w+) (\d+)", header))
    assert {k: int(v) for k, v in limits.items()} == {
        "MIN_SIDE": _lib.PP_MIN_SIDE, "MAX_SIDE": _lib.PP_MAX_SIDE, "MAX_MARGIN": _lib.PP_MAX_MARGIN, "MAX_BATCH": _lib.PP_MAX_BATCH,
        "NO_BBOX": _lib.PP_NO_BBOX, "DEGENERATE": _lib.PP_DEGENERATE, "OVERFLOW": _lib.PP_OVERFLOW}
    assert (PC.MIN_SIDE, PC.MAX_SIDE, PC.MAX_MARGIN) == (_lib.PP_MIN_SIDE, _lib.PP_MAX_SIDE, _lib.PP_MAX_MARGIN) == (16, 1024, 64)
    assert (PC.NO_BBOX, PC.DEGENERATE, PC.OVERFLOW) == (preprocess.NO_BBOX, preprocess.DEGENERATE, preprocess.OVERFLOW) == (1, 2, 4)
    fields = re.search(r"typedef struct siggan_preprocess_options \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"int32_t (\w+);", fields) == [n for n, _ in _lib.PreprocessOptions._fields_]
    assert C.sizeof(_lib.PreprocessOptions) == 24
    plan = open(os.path.join(CSRC, "preprocess_plan.h")).read()
    assert "PP_MIN_SIDE = 16, PP_MAX_SIDE = 1024, PP_MAX_MARGIN = 64, PP_MAX_BATCH = 65536" in plan


def test_the_new_table_is_bound_beside_the_pinned_registry():
    assert _lib.EXTRA_GROUPS == (_lib._PREPROCESS_SIGNATURES,)
    assert len(_lib.GROUPS) == 18 and _lib.ALL_EXPORTS[-1] == "siggan_dtw_pairs" and len(_lib.ALL_EXPORTS) == sum(len(g) for g in _lib.GROUPS)
    assert not any("preprocess" in name for name in _lib.ALL_EXPORTS)
    assert not any(g is _lib._PREPROCESS_SIGNATURES for g in _lib.GROUPS)
    assert not [n for n in vars(_lib) if re.fullmatch(r"[A-Z_]*EXPORTS", n) and "PREPROCESS" in n]
    assert _lib.EXTRA_SYMBOLS == tuple(_lib._PREPROCESS_SIGNATURES)
    lib = _lib.load()
    for name, (res, args) in _lib._PREPROCESS_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert _lib.ABI_VERSION == 4 and lib.siggan_abi_version() == 4
    src = re.search(r"^SRC = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1).split()
    assert "preprocess.hip" in src and src.index("preprocess.hip") == src.index("dtw.hip") + 1


def test_the_workspace_size():
    lib = _lib.load()
    for total, n in ((256, 1), (1 << 20, 1), (12345, 7), (2048 * 1024 * 1024, 2048)):
        want = ((total + 7) & ~7) + 8 * ((total >> 6) + 1024 * n) + 2 * 4 * ((total >> 1) + 1024 * n) + 4 * 256 * n + 4 * 8 * n
        assert lib.siggan_preprocess_workspace(total, n) == want == preprocess.workspace_bytes(total, n)
    assert lib.siggan_preprocess_workspace(0, 1) == 0 and lib.siggan_preprocess_workspace(256, 0) == 0
    assert lib.siggan_preprocess_workspace(256, _lib.PP_MAX_BATCH + 1) == 0


def test_the_geometry_header_under_sanitizers(tmp_path):
    """csrc/preprocess_plan.h -- where each scan's row masks and run slots lie in the workspace, and what a geometry table
    must satisfy -- by the stand-alone csrc/preprocess_plan_check.cpp under AddressSanitizer and UBSan: this is what the
    test is about, so it starts the compiler and the program."""
    exe = str(tmp_path / "preprocess_plan_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "preprocess_plan_check.cpp")],
                   check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert re.fullmatch(r"OK \d+", run.stdout.strip()) and int(run.stdout.split()[1]) > 8 * 1009 * 1009, run.stdout + run.stderr


# --------------------------------------------------------------------------------------------- the restatement by hand
def test_stage_1_on_inputs_worked_by_hand():
    g = np.full((16, 19), 77, dtype=np.uint8)
    assert (PC.blur(g) == 77).all() and (PC.denoise(g) == 77).all()
    g = np.zeros((16, 16), dtype=np.uint8)
    g[0, 0] = 160                                    # a corner: the reflection reads g[1][1], g[0][1], g[1][0], never g[0][0] twice
    b = PC.blur(g)
    assert b[0, 0] == (4 * 160 + 8) >> 4 and b[0, 1] == (2 * 160 + 8) >> 4 and b[1, 1] == (160 + 8) >> 4 and b[2, 2] == 0
    g = np.zeros((16, 16), dtype=np.uint8)
    g[1, 1] = 160                                    # ... and is read a second time from (-1, -1), (-1, 1), (1, -1)
    assert PC.blur(g)[0, 0] == (4 * 160 + 8) >> 4 and PC.blur(g)[0, 1] == (2 * 2 * 160 + 8) >> 4 and PC.blur(g)[1, 1] == (4 * 160 + 8) >> 4
    b = np.array([[5, 9], [1, 7]], dtype=np.uint8)
    e = PC.three(b, np.minimum)
    assert e.tolist() == [[5, 5], [1, 1]]            # (0, 0) sees itself only; (1, 1) sees 7, 9 above and 1 to the left
    assert PC.three(e, np.maximum).tolist() == [[5, 5], [5, 5]]
    b = np.array([[9, 9, 9], [9, 2, 9], [9, 9, 9]], dtype=np.uint8)
    assert PC.three(b, np.minimum).tolist() == [[9, 9, 9], [9, 2, 2], [9, 2, 9]]     # the element is {up, left, self}: it spreads down and right


def test_min_pixels_where_the_product_is_an_integer():
    for h, w in ((100, 100), (1000, 1000), (50, 20), (16, 125), (1024, 1024), (64, 64), (128, 128), (16, 16), (500, 2 * 16)):
        v = h * w * 0.001
        n = 0
        while not n > v:
            n += 1
        assert PC.min_pixels(h, w) == preprocess.default_min_pixels(h, w) == n, (h, w)
    assert PC.min_pixels(100, 100) == 11 and PC.min_pixels(50, 20) == 2 and PC.min_pixels(64, 64) == 5 and PC.min_pixels(16, 16) == 1
    assert PC.min_pixels(1000, 1000) == 1001 and PC.min_pixels(1024, 1024) == 1049


def test_resize_geometry_is_pythons_own_arithmetic():
    short = []
    for T in (64, 128):
        for cw in range(1, 1025):
            assert PC.resize_geometry(cw, cw, T) == (int(cw * (T / cw)),) * 2
            assert PC.resize_geometry(cw, 1, T)[0] == int(cw * min(T / cw, T / 1))
            if PC.resize_geometry(cw, cw, T)[0] != T:
                short.append((T, cw))
    assert PC.resize_geometry(49, 49, 64) == (int(49 * (64 / 49)),) * 2 == (63, 63)              # not simplified to T
    assert (64, 49) in short and all(PC.resize_geometry(cw, cw, T)[0] == T - 1 for T, cw in short)
    assert PC.resize_geometry(1024, 16, 64) == (64, 1) and PC.resize_geometry(1024, 15, 64) == (64, 0)
    assert PC.resize_geometry(16, 1024, 128) == (2, 128) and PC.resize_geometry(22, 19, 64) == (64, 55)


def test_the_box_average_by_hand():
    c = np.full((37, 53), 91, dtype=np.uint8)
    for nw, nh in ((64, 44), (5, 3), (53, 37), (1, 1)):
        assert (PC.box_resample(c, nw, nh) == 91).all()
    assert PC.box_resample(np.array([[0, 10, 20, 30]], dtype=np.uint8), 2, 1).tolist() == [[5, 25]]              # 2 : 1
    assert PC.box_resample(np.array([[0, 30, 60]], dtype=np.uint8), 2, 1).tolist() == [[10, 50]]                 # 3 : 2, weights 2 1 | 1 2
    assert PC.box_resample(np.array([[0, 31, 60]], dtype=np.uint8), 2, 1).tolist() == [[10, 50]]                 # 31 / 3 and 151 / 3, rounded
    assert PC.box_resample(np.array([[0, 1]], dtype=np.uint8), 1, 1).tolist() == [[1]]                           # a half rounds up
    assert PC.box_resample(np.array([[10, 50]], dtype=np.uint8), 3, 1).tolist() == [[10, 30, 50]]                # 2 : 3, upscaling by the same rule
    assert PC.box_resample(np.array([[0, 40], [80, 200]], dtype=np.uint8), 1, 1).tolist() == [[80]]
    assert PC.overlaps(3, 2).tolist() == [[2, 1, 0], [0, 1, 2]] and PC.overlaps(2, 3).tolist() == [[2, 0], [1, 1], [0, 2]]
    p = PC.paste(np.zeros((3, 5), dtype=np.uint8), 64)
    assert (p[30:33, 29:34] == 0).all() and int((p == 0).sum()) == 15


def test_centring_a_single_dot():
    canvas = np.full((64, 64), 255, dtype=np.uint8)
    canvas[10, 20] = 0
    out, sx, sy, m00 = PC.centre(canvas)
    assert (sx, sy, m00) == (12, 22, 255) and out[32, 32] == 0 and int((out != 255).sum()) == 1
    canvas[:] = 255
    canvas[63, 63] = 254                             # the faintest ink in the last corner: paper comes in from two sides
    out, sx, sy, m00 = PC.centre(canvas)
    assert (sx, sy, m00) == (-31, -31, 1) and out[32, 32] == 254 and (out[33:] == 255).all() and (out[:, 33:] == 255).all()
    blank = np.full((128, 128), 255, dtype=np.uint8)
    out, sx, sy, m00 = PC.centre(blank)
    assert (sx, sy, m00) == (0, 0, 0) and (out == 255).all()


def test_clahe_of_a_constant_takes_the_residual_path():
    tile = np.full((8, 8), 200, dtype=np.uint8)
    lut = PC.clahe_lut(tile, 1)                      # 64 pixels in one bin, clip 1: 63 clipped, batch 0, residual 63, step 4
    steps = np.zeros(256, dtype=np.int64)
    steps[np.arange(63) * 4] = 1
    steps[200] += 1
    want = np.minimum(PC.round_half_even_div(np.cumsum(steps) * 255, 64), 255)
    assert np.array_equal(lut, want) and int(steps.sum()) == 64 and int((steps[:249:4] >= 1).sum()) == 63 and steps[252] == 0
    assert lut[199] == 199 and lut[200] == 207 and lut[255] == 255       # 52 of 64 pixels at or below 200: 52 * 255 / 64 = 207.19
    assert (PC.clahe(np.full((64, 64), 200, dtype=np.uint8)) == 207).all()
    # T = 128: 256 pixels, clip 2: 254 clipped, batch 0, residual 254, step 1 -> bins 0..253 get one each
    lut = PC.clahe_lut(np.full((16, 16), 9, dtype=np.uint8), 2)
    assert lut[8] == PC.round_half_even_div(9 * 255, 256) and lut[9] == PC.round_half_even_div(12 * 255, 256) and lut[255] == 255


def test_clahe_of_all_distinct_values_and_against_floats():
    rng = np.random.RandomState(3)
    img = np.zeros((128, 128), dtype=np.uint8)
    for ty in range(8):
        for tx in range(8):
            img[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = rng.permutation(256).reshape(16, 16)
    lut = PC.round_half_even_div((np.arange(256) + 1) * 255, 256)        # nothing is clipped; every tile has this LUT
    assert np.array_equal(PC.clahe_lut(img[:16, :16], 2), lut) and np.array_equal(PC.clahe(img), lut[img].astype(np.uint8))
    assert lut[0] == 1 and lut[127] == 128 and lut[255] == 255           # 127.5 rounds to the even 128

    def clahe_floats(a):                             # the same rule in float64, where every product is exact
        T = a.shape[0]
        t = T // 8
        clip = max(int(2.0 * t * t / 256), 1)
        luts = [[PC.clahe_lut(a[y * t:(y + 1) * t, x * t:(x + 1) * t], clip).astype(np.float64) for x in range(8)] for y in range(8)]
        out = np.zeros_like(a)
        for y in range(T):
            ty = y / t - 0.5
            y1 = math.floor(ty)
            ya = ty - y1
            r1, r2 = max(y1, 0), min(y1 + 1, 7)
            for x in range(T):
                tx = x / t - 0.5
                x1 = math.floor(tx)
                xa = tx - x1
                c1, c2 = max(x1, 0), min(x1 + 1, 7)
                v = a[y, x]
                res = (luts[r1][c1][v] * (1 - xa) + luts[r1][c2][v] * xa) * (1 - ya) + (luts[r2][c1][v] * (1 - xa) + luts[r2][c2][v] * xa) * ya
                out[y, x] = int(np.rint(res))
        return out

    for T in (64, 128):
        a = PC.expected(T)[4]["canvas"]              # pen_200x333
        assert len(np.unique(a)) > 50 and np.array_equal(PC.clahe(a), clahe_floats(a))


def test_the_world_is_mostly_accepted_and_the_planted_cases_are_what_they_claim():
    names = [n for n, _ in PC.world()]
    assert len(names) == len(set(names))
    for T in (64, 128):
        res = PC.expected(T)
        rnd = [(n, a, r) for (n, a), r in zip(PC.world(), res) if PC.is_random(n)]
        good = sum(int(r["stats"][PC.STATUS] == 0 and PC.is_valid(int(r["stats"][PC.WHITE]), a.size)) for _, a, r in rnd)
        assert len(rnd) >= 12 and 4 * good >= 3 * len(rnd)
    shapes = {a.shape for _, a in PC.world()}
    assert {(16, 16), (17, 23), (64, 64), (65, 130), (200, 333), (1024, 16), (16, 1024), (1024, 1024), (300, 300)} <= shapes
    raw = {n: r["stats"] for (n, _), r in zip(PC.world(), PC.expected(64, denoise_on=False))}
    assert raw["blank"][PC.STATUS] == PC.NO_BBOX and raw["blank"][PC.COMPONENTS] == 0 and raw["blank"][PC.WHITE] == 64 * 64
    assert PC.min_pixels(100, 100) == 11 and raw["specks"][PC.COMPONENTS] == 7 and raw["specks"][PC.KEPT] == 1
    assert raw["specks"][PC.CROP_X:PC.CROP_H + 1].tolist() == [35, 25, 15, 13]                   # the one component of 11 pixels, margin 5
    assert raw["diagonal"][PC.COMPONENTS] == 1 and raw["diagonal"][PC.CROP_W] == 20
    assert raw["comb"][PC.COMPONENTS] == 1 and raw["spiral"][PC.COMPONENTS] == 1
    assert raw["borders"][PC.CROP_X:PC.CROP_H + 1].tolist() == [0, 0, 70, 90]
    assert raw["wide_line"][PC.STATUS] == PC.DEGENERATE and raw["threshold"][PC.COMPONENTS] > 1
    off = {n: r["stats"] for (n, _), r in zip(PC.world(), PC.expected(64, crop=False))}
    assert off["wide_line"][PC.NEW_H] == 1 and off["tall_texture"][PC.NEW_W] == 1 and (np.array([s[PC.COMPONENTS] for s in off.values()]) == 0).all()
    signs = {(int(np.sign(off[n][PC.SHIFT_X])), int(np.sign(off[n][PC.SHIFT_Y]))) for n in ("corner_tl", "corner_tr", "corner_bl", "corner_br")}
    assert signs == {(1, 1), (-1, 1), (1, -1), (-1, -1)}                                          # paper comes in from two sides, every pair
    tex = PC.world()[names.index("texture")][1]
    assert len(np.unique(tex)) == 256
    small = raw["small_crop"]
    assert small[PC.CROP_W] < 64 and small[PC.CROP_H] < 64 and small[PC.NEW_W] == 64
    v = PC.validity(np.stack([raw["blank"], raw["borders"]]), np.array([[0, 64, 64, 5], [0, 90, 70, 7]]))
    assert v.tolist() == [False, True] and preprocess.validity(np.stack([raw["blank"], raw["borders"]]), np.array([[0, 64, 64, 5], [0, 90, 70, 7]])).tolist() == [False, True]
    assert not PC.is_valid(951, 1000) and PC.is_valid(950, 1000) and PC.is_valid(0, 1000 * 1000)     # all ink passes, as in the reference


# ----------------------------------------------------------------------------------------------------------- refusals
def cpu_batch(n=2, side=16):
    geom = torch.tensor([[i * side * side, side, side, 1] for i in range(n)], dtype=torch.int64)
    return preprocess.ScanBatch(torch.zeros(n * side * side, dtype=torch.uint8), geom.clone(), geom, torch.zeros(8, dtype=torch.uint8))


def test_the_python_layer_refuses_in_order_and_in_these_words():
    ok = np.zeros((16, 16), dtype=np.uint8)
    for scans, kw, words in [
            (ok, {}, "scans must be a list of \\(h, w\\) uint8 arrays, got ndarray"),
            ([], {}, "scans holds no scan"),
            ([ok, "x"], {}, "scan 1 must be a numpy array or a tensor, got str"),
            ([ok, ok.astype(np.float32)], {}, "scan 1 must be uint8, got float32"),
            ([ok[0]], {}, "scan 0 must be \\(h, w\\), got \\(16,\\)"),
            ([np.zeros((15, 16), np.uint8)], {}, "scan 0: height = 15 outside \\[16, 1024\\]"),
            ([ok, np.zeros((16, 1025), np.uint8)], {}, "scan 1: width = 1025 outside \\[16, 1024\\]"),
            ([ok], dict(min_pixels=0), "scan 0: min_pixels = 0 < 1"),
            ([ok], dict(min_pixels=1.5), "min_pixels must be an integer"),
            ([ok], dict(min_pixels=[1, 2]), "min_pixels holds 2 values for 1 scans"),
            ([np.zeros((15, 16), np.float32)], {}, "must be uint8"),                             # dtype before sizes
            ([ok], dict(device="cpu"), "no CPU path")]:
        with pytest.raises(ValueError, match=words):
            preprocess.pack_scans(scans, **kw)
    b = cpu_batch()
    for args, kw, words in [
            (("x",), {}, "batch must be a ScanBatch \\(pack_scans\\), got str"),
            ((b,), dict(size=96), "size must be 64 or 128, got 96"),
            ((b,), dict(size=64.0), "size must be an integer"),
            ((b,), dict(margin=-1), "margin = -1 outside \\[0, 64\\]"),
            ((b,), dict(margin=65), "margin = 65 outside \\[0, 64\\]"),
            ((b,), dict(size=32, margin=99), "size must be 64 or 128"),                          # parameters in the order given
            ((b,), {}, "batch must live on a ROCm device .*no CPU path")]:
        with pytest.raises(ValueError, match=words):
            preprocess.preprocess_scans(*args, **kw)
    with pytest.raises(ValueError, match="target_size must be \\(64, 64\\) or \\(128, 128\\), got \\(64, 128\\)"):
        preprocess_signatures.preprocess_single_image("nowhere.png", target_size=(64, 128))
    with pytest.raises(NotImplementedError, match="not implemented here"):
        preprocess_signatures.preprocess_single_image("nowhere.png", binarize=True)
    with pytest.raises(NotImplementedError, match="adaptiveThreshold"):
        preprocess_signatures.preprocess_batch("nowhere", "nowhere_out", binarize=True)
    assert preprocess_signatures.preprocess_single_image("nowhere.png") is None                  # unreadable: None before any device


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)                   # host memory: a refused call reads none of it
    p = C.c_void_p(buf.ctypes.data)
    good_geom = np.array([[0, 16, 16, 1], [256, 16, 20, 2]], dtype=np.int64)
    total = 256 + 320
    need = lib.siggan_preprocess_workspace(total, 2)

    def call(geom=good_geom, n=2, total=total, opt=(64, 1, 1, 1, 1, 5), ws_bytes=need, **k):
        geom = np.ascontiguousarray(geom, dtype=np.int64)
        g = C.c_void_p(geom.ctypes.data)
        o = _lib.PreprocessOptions(*opt)
        rc = lib.siggan_preprocess_u8(0, k.get("pool", p), total, k.get("geom_host", g), k.get("geom_dev", p), n,
                                      k.get("options", o), k.get("out", p), k.get("stats", p), None, None, k.get("ws", p), ws_bytes, None)
        return rc, lib.siggan_last_error().decode()

    def with_row(i, col, v):
        g = good_geom.copy()
        g[i, col] = v
        return g

    for kw, words in [
            (dict(n=0), "n = 0 outside [1, 65536]"),
            (dict(n=65537), "n = 65537 outside [1, 65536]"),
            (dict(pool=None), "null pool_dev"),
            (dict(geom_host=None), "null geometry table"),
            (dict(geom_dev=None), "null geometry table"),
            (dict(options=None), "null options"),
            (dict(out=None), "missing out_dev"),
            (dict(stats=None), "missing stats_dev"),
            (dict(ws=None), "null workspace_dev"),
            (dict(opt=(96, 1, 1, 1, 1, 5)), "target must be 64 or 128, got 96"),
            (dict(opt=(64, 1, 1, 1, 1, -1)), "margin = -1 outside [0, 64]"),
            (dict(opt=(128, 1, 1, 1, 1, 65)), "margin = 65 outside [0, 64]"),
            (dict(geom=with_row(1, 1, 15)), "scan 1: height = 15 outside [16, 1024]"),
            (dict(geom=with_row(0, 1, 1025)), "scan 0: height = 1025 outside [16, 1024]"),
            (dict(geom=with_row(1, 2, 15)), "scan 1: width = 15 outside [16, 1024]"),
            (dict(geom=with_row(1, 2, 1025)), "scan 1: width = 1025 outside [16, 1024]"),
            (dict(geom=with_row(1, 3, 0)), "scan 1: min_pixels = 0 < 1"),
            (dict(geom=with_row(0, 0, -1)), "scan 0: offset = -1 < 0"),
            (dict(geom=with_row(1, 0, 255)), "scan 1: offset = 255 overlaps the scan before it"),
            (dict(geom=good_geom[::-1]), "scan 1: offset = 0 overlaps the scan before it"),
            (dict(geom=with_row(1, 0, 257)), "scan 1: offset = 257 + 16 x 20 runs past total_pixels = 576"),
            (dict(total=575), "runs past total_pixels = 575"),
            (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes is too small: {need} needed"),
            (dict(ws=C.c_void_p(buf.ctypes.data + 4)), "workspace_dev must be 8-byte aligned"),
            (dict(stats=C.c_void_p(buf.ctypes.data + 2)), "stats_dev must be 4-byte aligned")]:
        rc, msg = call(**kw)
        assert rc == _lib.E_ARG and words in msg, (kw, msg)
    assert not buf.any()


# ------------------------------------------------------------------------------------------------------ command lines
def test_the_cli_has_the_references_flags_and_binarize_exits(capsys, tmp_path):
    p = preprocess_signatures.build_parser()
    flags = sorted(s for a in p._actions for s in a.option_strings)
    assert flags == sorted(["-h", "--help", "--size", "--binarize", "--no-crop", "--no-center", "--no-denoise", "--no-validate", "--verbose", "-v"])
    assert [a.dest for a in p._actions if not a.option_strings] == ["input_dir", "output_dir"]
    a = p.parse_args(["in", "out"])
    assert (a.size, a.binarize, a.no_crop, a.no_center, a.no_denoise, a.no_validate, a.verbose) == (64, False, False, False, False, False, False)
    assert p.parse_args(["in", "out", "--size", "128", "-v"]).size == 128
    with pytest.raises(SystemExit):
        p.parse_args(["in", "out", "--size", "96"])
    with pytest.raises(SystemExit) as e:
        preprocess_signatures.main([str(tmp_path), str(tmp_path / "out"), "--binarize"])
    assert e.value.code not in (0, None) and "--binarize is not implemented here" in str(e.value.code) and "\n" not in str(e.value.code)
    assert "adaptiveThreshold" in str(e.value.code) and not (tmp_path / "out").exists()
    preprocess_signatures.print_summary(3, 12, [f"f{i}.png" for i in range(12)])
    assert capsys.readouterr().out == ("\n" + "=" * 50 + "\nPreprocessing Complete\n" + "=" * 50 + "\nSuccessfully processed: 3\nFailed: 12\n"
                                       "\nFailed files:\n" + "".join(f"  - f{i}.png\n" for i in range(10)) + "  ... and 2 more\n")
    preprocess_signatures.print_summary(1, 0, [])
    assert capsys.readouterr().out == "\n" + "=" * 50 + "\nPreprocessing Complete\n" + "=" * 50 + "\nSuccessfully processed: 1\nFailed: 0\n"


def test_the_modules_host_helpers():
    ps = preprocess_signatures
    assert (ps.DEFAULT_TARGET_SIZE, ps.DEFAULT_MARGIN, ps.DEFAULT_BINARY_THRESHOLD) == ((64, 64), 5, 127)
    assert (ps.MIN_CONTOUR_AREA_RATIO, ps.MAX_NOISE_RATIO, ps.MIN_INK_RATIO) == (0.001, 0.95, 0.01)
    assert ps.EXTENSIONS == ('.png', '.jpg', '.jpeg', '.bmp', '.tiff')
    a = np.array([[0, 127, 128, 255]], dtype=np.uint8)
    n = ps.normalize_pixels(a)
    assert n.dtype == np.float32 and n[0, 0] == -1.0 and n[0, 3] == 1.0 and np.array_equal(ps.denormalize_pixels(n)[0, [0, 3]], [0, 255])
    assert ps.normalize_pixels(a, (0.0, 1.0))[0, 3] == 1.0
    assert ps.create_preprocessing_config() == {'target_size': (64, 64), 'binarize': False, 'remove_margin': True, 'center': True,
                                                'denoise': True, 'validate': True}
    img = np.full((10, 10), 255, dtype=np.uint8)
    assert not ps.is_valid_signature(img)
    img[0, :5] = 127
    assert ps.is_valid_signature(img)                # 127 is ink: 95 % white is not more than 95 %
    img[0, 4] = 128
    assert not ps.is_valid_signature(img)            # 128 is white: 96 %
    assert ps.is_valid_signature(img, max_noise_ratio=0.96) and not ps.is_valid_signature(img, 0.05, 0.99)


def test_generate_signatures_parses_the_preprocess_flags_and_keeps_its_defaults():
    from signature_gan_amd import generate_signatures as gen
    base = ["--checkpoint", "x.pth"]
    a = gen.parse_args(base)
    assert "adapt_preprocess" not in vars(a) and "project_preprocess" not in vars(a)             # a command line without them parses to what it did
    assert not gen.preprocess_opt(a, "adapt_preprocess") and not gen.preprocess_opt(a, "project_preprocess")
    assert gen.preprocess_opt(gen.parse_args(base + ["--adapt", "dir", "--adapt_preprocess"]), "adapt_preprocess") is True
    assert gen.preprocess_opt(gen.parse_args(base + ["--project", "dir", "--project_preprocess"]), "project_preprocess") is True
    for bad in (["--adapt_preprocess"], ["--project_preprocess"], ["--adapt", "d", "--project_preprocess"], ["--project", "d", "--adapt_preprocess"]):
        with pytest.raises(SystemExit):
            gen.parse_args(base + bad)
