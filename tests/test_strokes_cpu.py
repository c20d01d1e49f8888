"""Stroke geometry without a device: what the numpy restatement (tests/strokescommon.py) itself satisfies on exactly the inputs
the GPU tests use, the metric's arithmetic, the refusals, the constants and the two CLIs' new flags.

The GPU tests demand that a redraw at radius 0 fed back is a fixed point reached in one pass, that the all-ink 128 x 128 image
needs 65 passes and that the number of 8-connected components survives the thinning; here the reference alone is shown to meet
all of that, so a device result equal to the reference meets it too."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import strokescommon as SC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, strokes
from signature_gan_amd.utils import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_inputs():
    """Every image the GPU tests launch, as (name, uint8 image)."""
    for h, w in SC.GPU_SHAPES:
        for name, img in SC.fills(h, w).items():
            yield f"{h}x{w}/{name}", img
        for name, img in SC.edges(h, w).items():
            yield f"{h}x{w}/{name}", img


def test_a_2x2_block_thins_to_one_pixel():
    g = np.zeros((6, 8), dtype=bool)
    g[2:4, 2:4] = True
    skel, passes = SC.thin(g)
    assert skel.sum() == 1 and passes == 2
    stats, _, skel, _ = SC.reference(SC.edges(64, 64)["block_2x2"])
    assert stats[SC.INK] == 4 and stats[SC.SKELETON] == 1 and skel.sum() == 1
    assert stats[SC.ENDPOINTS] == 0 and stats[SC.D2_MAX] == 1 and stats[SC.WIDTH_HIST] == 1


def test_a_skeleton_is_a_fixed_point_reached_in_one_pass_and_keeps_the_components():
    n = 0
    for name, img in gpu_inputs():
        mask, stats, d2, skel = SC.geometry(img)
        sk = skel.astype(bool)
        assert not (sk & ~mask).any(), name
        again, passes = SC.thin(sk)
        assert passes == 1 and np.array_equal(again, sk), name
        assert SC.components8(mask) == SC.components8(sk), name
        assert 1 <= stats[SC.PASSES] <= max(img.shape) // 2 + 2, name
        assert stats[SC.WIDTH_HIST:].sum() == stats[SC.SKELETON] and d2.max() <= 4096 and d2.min() >= 0
        n += 1
    assert n >= 110


def test_full_rectangles_need_at_most_half_the_longer_side_plus_two_passes():
    for h in (1, 2, 3, 5, 33, 64, 127, 128):
        for w in (4, 8, 12, 64, 68, 124, 128):
            _, passes = SC.thin(np.ones((h, w), dtype=bool))
            assert passes <= max(h, w) // 2 + 2, (h, w, passes)
    assert SC.thin(np.ones((128, 128), dtype=bool))[1] == 65
    assert SC.reference(SC.edges(128, 128)["all_ink"])[0][SC.PASSES] == 65
    assert SC.reference(SC.edges(128, 128)["all_ink"])[0][SC.D2_MAX] == 64 * 64


def test_a_bar_of_width_w_lands_in_bin_ceil_w_over_2():
    for width in range(1, 9):
        stats = SC.reference(SC.bar(width))[0]
        hist = stats[SC.WIDTH_HIST:]
        k = (width + 1) // 2
        assert hist[k - 1] > 30 and hist[k - 1] >= 0.8 * hist.sum(), (width, hist)      # the two line ends apart
        assert hist[k:].sum() == 0, (width, hist)
    assert SC.width_bins(np.array([1, 2, 4, 5, 9, 10, 225, 226, 4096])).tolist() == [1, 2, 2, 3, 3, 4, 15, 16, 16]


def test_distance_map_is_exact_against_brute_force():
    img = SC.fills(33, 64)["blurred_noise"]
    mask = img < 128
    padded = np.pad(mask, 1)
    by, bx = np.nonzero(~padded)
    want = np.zeros(mask.shape, dtype=np.int64)
    for y, x in zip(*np.nonzero(mask)):
        want[y, x] = ((by - (y + 1)) ** 2 + (bx - (x + 1)) ** 2).min()
    assert np.array_equal(SC.distance2(mask), want)
    assert np.array_equal(SC.dilate(mask, 0), mask) and SC.dilate(mask, 1).sum() > mask.sum()


def test_the_kernels_word_arithmetic_equals_a_per_pixel_restatement_on_the_host(tmp_path):
    """csrc/strokes_word.h -- what k_strokes computes with, compiled for the host -- run as the kernel runs it (one word per
    thread, ping-pong buffers, a flag word per pass) by the stand-alone csrc/strokes_word_check.cpp, under AddressSanitizer and
    UBSan: this is what the test is about, so it starts the compiler and the program."""
    import subprocess
    csrc = os.path.join(ROOT, "signature-gan_amd", "csrc")
    exe = str(tmp_path / "strokes_word_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(csrc, "strokes_word_check.cpp")],
                   check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "OK 300 cases, max passes 65", run.stdout + run.stderr     # 65: the full 128 x 128 image


def test_stroke_geometry_arithmetic():
    c = np.zeros((4, 23), dtype=np.int32)
    #        ink skel ends junc passes d2max d2sum
    c[0, :7] = [100, 20, 2, 1, 3, 9, 50]
    c[0, SC.WIDTH_HIST:SC.WIDTH_HIST + 3] = [10, 6, 4]                           # widths 1, 3, 5
    c[1, :7] = [0, 0, 0, 0, 1, 0, 0]                                             # an empty image
    c[2, :7] = [30, 10, 4, 0, 2, 5, 12]
    c[2, SC.WIDTH_HIST + 1] = 10
    c[3, :7] = [0, 0, 0, 0, -1, 0, 0]                                            # the bound was hit
    d = metrics.stroke_geometry_from_counters(c)
    assert d["images"] == 4 and d["empty"] == 1 and d["bound_hit"] == 1
    assert d["width_histogram"] == [10, 16, 4] + [0] * 13
    assert d["mean_width"] == (10 * 1 + 16 * 3 + 4 * 5) / 30
    per = np.array([(10 + 18 + 20) / 20, 3.0])
    assert d["width_per_image"] == {"mean": float(per.mean()), "std": float(per.std())}
    assert d["thickest"] == {"mean": (5 + 5) / 2, "max": 5}                      # ceil(sqrt(9)) = 3, ceil(sqrt(5)) = 3
    assert d["skeleton_length"] == {"mean": 10.0, "std": float(np.std([20, 0, 10]))}
    assert d["endpoints"] == {"mean": 2.0} and d["junction_pixels"] == {"mean": 1 / 3}
    assert d["ink_per_skeleton_pixel"] == {"mean": (5.0 + 3.0) / 2}
    none = metrics.stroke_geometry_from_counters(c[1:2])
    assert none["mean_width"] is None and none["width_per_image"] == {"mean": None, "std": None}
    assert none["thickest"] == {"mean": None, "max": None} and none["ink_per_skeleton_pixel"] == {"mean": None}
    assert none["skeleton_length"] == {"mean": 0.0, "std": 0.0} and none["empty"] == 1
    with pytest.raises(ValueError):
        metrics.stroke_geometry_from_counters(np.zeros((0, 23), np.int32))
    assert metrics._ceil_sqrt(np.array([0, 1, 2, 4, 5, 4095, 4096])).tolist() == [0, 1, 2, 2, 3, 64, 64]
    # on the reference's counters of a bar: width 5 reads 5, width 4 reads 3
    for width, reads in ((5, 5), (4, 3)):
        g = metrics.stroke_geometry_from_counters(SC.reference(SC.bar(width))[0][None])
        assert g["thickest"] == {"mean": float(reads), "max": reads} and abs(g["mean_width"] - reads) < 0.5


def test_refusals_that_need_no_device_and_their_order():
    ok = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for images, kw, what in [(np.zeros((2, 8, 8), np.uint8), {}, "tensor"), (ok.float(), {}, "uint8"), (ok[0], {}, r"\(N, H, W\)"),
                             (torch.zeros(2, 2, 8, 8, dtype=torch.uint8), {}, r"\(N, H, W\)"),
                             (torch.zeros(2, 0, 8, dtype=torch.uint8), {}, "height"), (torch.zeros(2, 129, 8, dtype=torch.uint8), {}, "height"),
                             (torch.zeros(2, 8, 6, dtype=torch.uint8), {}, "width"), (torch.zeros(2, 8, 132, dtype=torch.uint8), {}, "width"),
                             (torch.zeros(2, 8, 0, dtype=torch.uint8), {}, "width"), (ok, dict(threshold=0), "threshold"),
                             (ok, dict(threshold=256), "threshold"), (ok, dict(threshold=1.5), "threshold"), (ok, dict(threshold=True), "threshold")]:
        for fn in (strokes.stroke_stats, strokes.distance_map, strokes.skeleton_u8):
            with pytest.raises(ValueError, match=what):
                fn(images, **kw)
    for kw, what in ((dict(radius2=-1), "radius2"), (dict(radius2=37), "radius2"), (dict(radius2=1.0), "radius2"), (dict(radius2=0, ink=128), "ink"),
                     (dict(radius2=0, ink=-1), "ink"), (dict(radius2=0, fill=127), "fill"), (dict(radius2=0, fill=256), "fill"),
                     (dict(radius2=0, threshold=200, fill=199), "fill"), (dict(radius2=0, threshold=50, ink=50), "ink")):
        with pytest.raises(ValueError, match=what):
            strokes.restroke_u8(ok, **kw)
    # the order: dtype before sizes, sizes before parameters, threshold before radius2 before ink before fill, all before the device
    with pytest.raises(ValueError, match="uint8"):
        strokes.stroke_stats(torch.zeros(2, 129, 6), threshold=0)
    with pytest.raises(ValueError, match="height"):
        strokes.stroke_stats(torch.zeros(2, 129, 6, dtype=torch.uint8), threshold=0)
    with pytest.raises(ValueError, match="width"):
        strokes.stroke_stats(torch.zeros(2, 8, 6, dtype=torch.uint8), threshold=0)
    with pytest.raises(ValueError, match="threshold"):
        strokes.restroke_u8(ok, 99, threshold=0, ink=-1, fill=0)
    with pytest.raises(ValueError, match="radius2"):
        strokes.restroke_u8(ok, 99, ink=-1, fill=0)
    with pytest.raises(ValueError, match="ink"):
        strokes.restroke_u8(ok, 0, ink=-1, fill=0)
    for fn in (strokes.stroke_stats, strokes.distance_map, strokes.skeleton_u8, lambda x: strokes.restroke_u8(x, 0)):
        with pytest.raises(ValueError, match="no CPU path"):                     # every argument fine but the device
            fn(ok)
    assert [strokes.radius2_for_pen_width(w) for w in range(1, 10)] == [0, 0, 1, 2, 4, 6, 9, 12, 16]
    for bad in (0, 10, 2.0, True):
        with pytest.raises(ValueError):
            strokes.radius2_for_pen_width(bad)


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)                                                 # host memory: a refused call reads none of it
    p = C.c_void_p(buf.ctypes.data)
    odd = lambda n: C.c_void_p(buf.ctypes.data + n)                              # noqa: E731
    call = lambda **k: lib.siggan_strokes_u8(0, k.get("u8", p), k.get("batch", 1), k.get("h", 4), k.get("w", 4), k.get("thr", 128),   # noqa: E731
                                             k.get("r2", 0), k.get("ink", 0), k.get("fill", 255), k.get("stats", p), k.get("d2", None),
                                             k.get("skel", None), k.get("redraw", None), None)
    for bad in (dict(batch=0), dict(h=0), dict(h=129), dict(w=2), dict(w=10), dict(w=132), dict(thr=0), dict(thr=256), dict(r2=-1), dict(r2=37),
                dict(ink=-1), dict(ink=128), dict(fill=127), dict(fill=256), dict(stats=None), dict(u8=None), dict(u8=odd(2)), dict(stats=odd(2)),
                dict(d2=odd(1)), dict(skel=odd(2)), dict(redraw=odd(1))):
        assert call(**bad) == _lib.E_ARG, bad
        assert lib.siggan_last_error()


def test_header_constants_equal_the_python_ones_and_the_symbol_is_exported():
    text = open(os.path.join(ROOT, "include", "siggan_strokes.h")).read()
    define = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))          # noqa: E731
    assert define("SIGGAN_SK_MAX_SIZE") == _lib.SK_MAX_SIZE == 128
    assert define("SIGGAN_SK_WIDTH_BINS") == _lib.SK_WIDTH_BINS == strokes.WIDTH_BINS == SC.WIDTH_BINS == 16
    assert define("SIGGAN_SK_MAX_RADIUS2") == _lib.SK_MAX_RADIUS2 == 36 >= strokes.radius2_for_pen_width(strokes.MAX_PEN_WIDTH)
    names = re.findall(r"^\s+SIGGAN_SK_([A-Z0-9_]+)\b", text[text.index("enum {"):text.index("SIGGAN_SK_COUNT")], flags=re.M)
    assert names == ["INK", "SKELETON", "ENDPOINTS", "JUNCTION_PIXELS", "PASSES", "D2_MAX", "D2_SKEL_SUM", "WIDTH_HIST"]
    assert [getattr(strokes, n) for n in names] == list(range(8)) == [getattr(SC, n) for n in names]
    assert _lib.SK_COUNT == strokes.COUNT == SC.COUNT == len(strokes.STAT_NAMES) == 23
    assert strokes.STAT_NAMES[:7] == tuple(n.lower() for n in names[:7]) and strokes.STAT_NAMES[7] == "width_hist_1"
    assert _lib.STROKES_EXPORTS == ("siggan_strokes_u8",)
    assert hasattr(_lib.load(), "siggan_strokes_u8")
    assert _lib.ABI_VERSION == 4 and _lib.load().siggan_abi_version() == 4


def test_both_clis_parse_the_new_flags_and_keep_their_defaults():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import generate_signatures as gen
    base = ["--checkpoint", "x.pth"]
    a = ev.parse_args(base)
    assert a.strokes is False and "strokes" not in vars(a)                       # a command line without it parses to what it did
    assert ev.parse_args(base + ["--strokes"]).strokes is True
    g = gen.parse_args(base)
    assert "pen_width" not in vars(g) and gen.pen_width_opt(g) is None and gen.with_pen_width(None) == {}
    pw = gen.pen_width_opt(gen.parse_args(base + ["--pen_width", "5"]))
    assert pw.report() == {"pen_width": 5, "radius2": 4, "threshold": 128, "mean_width_before": None, "mean_width_after": None}
    pw = gen.pen_width_opt(gen.parse_args(base + ["--pen_width", "3", "--threshold", "100", "--despeckle", "6"]))
    assert (pw.width, pw.radius2, pw.threshold) == (3, 1, 100)
    for bad in (["--pen_width", "0"], ["--pen_width", "10"], ["--pen_width", "3", "--filter_by_realism"],
                ["--pen_width", "3", "--refine_by_realism"], ["--pen_width", "3", "--adapt", "dir"], ["--pen_width", "3", "--project", "p"],
                ["--pen_width", "3", "--morph"], ["--pen_width", "3", "--threshold", "0"], ["--pen_width"]):
        with pytest.raises(SystemExit):
            gen.parse_args(base + bad)
    pw.before += np.array([4, 4] + [0] * 14)
    pw.after += np.array([0, 8] + [0] * 14)
    assert (pw.report()["mean_width_before"], pw.report()["mean_width_after"]) == (2.0, 3.0)
    # the summary prints its stroke-geometry lines only when the key is there
    import contextlib
    import io
    out = io.StringIO()
    m = {"n_samples": 1, "image_shape": [1, 64, 64]}
    with contextlib.redirect_stdout(out):
        ev.print_summary(m)
    assert "Stroke geometry" not in out.getvalue()
    geo = metrics.stroke_geometry_from_counters(SC.reference(SC.bar(5))[0][None])
    with contextlib.redirect_stdout(out):
        ev.print_summary(dict(m, stroke_geometry={"threshold": 128, "generated": geo}))
    assert "Stroke geometry" in out.getvalue() and "Generated: pen width" in out.getvalue()
