"""Connected components without a device: the yardstick, an independent restatement, the lock-step emulation of the kernel's
method (tests/componentscommon.py), the metric's arithmetic, the refusals and the two CLIs' new flags.

The emulation runs csrc/components.hip's union-find with its data structures and 512 threads in lock step.  Its bounds are the
kernel's: a find walks a chain of strictly decreasing slots, so fewer than `nodes` = h * w / 2 steps; a join retries only after
another thread re-pointed its larger root to something smaller, so at most 2 * nodes times.  What it records at 128 x 128
(8-connectivity, thread order): checkerboard 8192 runs, longest chain 27, 2 retries, 253 ticks; column serpentine 8129 runs,
chain 13, 1 retry; spiral 4097 runs, chain 13; row serpentine 128 runs, chain 8; comb 8129 runs, chain 8, 804 ticks -- two to
three orders of magnitude under the bounds of 8192 / 16384."""
import ctypes as C

import numpy as np
import pytest
import torch

import componentscommon as CC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, components
from signature_gan_amd.utils import metrics

WORST = ("checkerboard", "serpentine", "serpentine_columns", "spiral", "comb", "u_ring_arch", "noise_0.5", "word_border")


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("shape", CC.GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flood_fill_and_emulation_equal_scipy_on_every_case(shape, conn):
    h, w = shape
    ma = CC.default_min_area(h, w)
    fam = CC.families(h, w)
    assert len(fam) >= 19
    worst = {"find_steps": 0, "retries": 0, "ticks": 0}
    for name, img in fam.items():
        want = CC.yardstick(img, 128, conn, ma, 255)
        assert same(CC.flood(img, 128, conn, ma, 255), want), name
        got = CC.emulate(img, 128, conn, ma, 255)
        info = got[3]
        assert not info["bound_hit"] and got[0][CC.COMPONENTS] >= 0, name
        assert same(got, want), (name, got[0], want[0])
        assert info["find_steps"] < info["nodes"] and info["retries"] <= 2 * info["nodes"]
        assert info["runs"] <= info["nodes"] == h * w // 2
        for k in worst:
            worst[k] = max(worst[k], info[k])
    print(f"{h}x{w} conn {conn}: longest chain {worst['find_steps']}, most retries {worst['retries']}, most ticks {worst['ticks']} "
          f"(bounds {h * w // 2} / {h * w})")


@pytest.mark.parametrize("order", ["reverse", 1, 2])
@pytest.mark.parametrize("shape", [(64, 64), (128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_the_emulations_result_does_not_depend_on_the_order_of_the_threads(shape, order):
    h, w = shape
    fam = CC.families(h, w)
    for name in WORST:
        for conn in (8, 4):
            want = CC.yardstick(fam[name], 128, conn, 3, 200)
            got = CC.emulate(fam[name], 128, conn, 3, 200, order=order)
            assert not got[3]["bound_hit"] and same(got, want), (name, conn)
            assert got[3]["find_steps"] < got[3]["nodes"] and got[3]["retries"] <= 2 * got[3]["nodes"]


def test_case_families_are_what_they_claim():
    fam = CC.families(128, 128)
    ys = lambda name, conn, ma=1: CC.yardstick(fam[name], 128, conn, ma, 255)[0]      # noqa: E731
    assert ys("empty", 8).tolist() == [0, 0, 0, 0, 0, -1, -1, -1, -1]
    assert ys("full", 4).tolist() == [16384, 1, 16384, 0, 0, 0, 0, 127, 127]
    assert ys("corners", 8)[CC.COMPONENTS] == 4
    assert ys("diagonal_pair", 8)[CC.COMPONENTS] == 1 and ys("diagonal_pair", 4)[CC.COMPONENTS] == 2
    assert ys("checkerboard", 8)[CC.COMPONENTS] == 1 and ys("checkerboard", 4)[CC.COMPONENTS] == 128 * 128 // 2
    for name in ("serpentine", "serpentine_columns", "spiral", "comb"):
        assert ys(name, 4)[CC.COMPONENTS] == 1 and ys(name, 4)[CC.INK] > 8000, name
    ma = CC.default_min_area(128, 128)
    s = ys("around_min_area", 4, ma)
    assert s[CC.COMPONENTS] == 3 and s[CC.SMALL_COMPONENTS] == 1 and s[CC.SMALL_INK] == ma - 1 and s[CC.LARGEST] == ma + 1
    grey = fam["strokes"]
    assert (grey < 128).any() and (grey >= 128).any() and len(np.unique(grey)) > 16
    assert CC.default_min_area(64, 64) == components.default_min_area(64, 64) == 4 and components.default_min_area(128, 128) == 16
    assert components.default_min_area(8, 8) == 2


def test_fragmentation_arithmetic():
    #            ink comps largest small small_ink box
    c = np.array([[100, 5, 80, 3, 6, 0, 0, 9, 9],
                  [0, 0, 0, 0, 0, -1, -1, -1, -1],
                  [50, 2, 40, 1, 10, 1, 1, 5, 5],
                  [10, 10, 1, 10, 10, -1, -1, -1, -1]], dtype=np.int32)
    d = metrics.fragmentation_from_counters(c)
    assert d["n"] == 4 and d["empty_images"] == 1
    assert d["components_mean"] == 17 / 4 and d["components_median"] == 3.5 and d["small_components_mean"] == 14 / 4
    assert d["speckle_ink_ratio"] == 26 / 160
    assert d["largest_component_share_mean"] == float(np.mean(np.array([80, 40, 1]) / np.array([100, 50, 10])))
    empty = metrics.fragmentation_from_counters(c[1:2])
    assert empty["speckle_ink_ratio"] == 0.0 and empty["largest_component_share_mean"] is None and empty["empty_images"] == 1
    with pytest.raises(ValueError):
        metrics.fragmentation_from_counters(np.zeros((0, 9), np.int32))
    bad = c.copy(); bad[0, 1] = -1
    with pytest.raises(RuntimeError):
        metrics.fragmentation_from_counters(bad)
    x = torch.tensor([-1.0, -0.5, 0.0, 0.999, 1.0, 3.0])
    assert metrics.quantize_generated(x).tolist() == [0, 63, 127, 254, 255, 255]


def test_refusals_that_need_no_device():
    ok = torch.zeros(2, 8, 8, dtype=torch.uint8)
    for images, kw in [(np.zeros((2, 8, 8), np.uint8), {}), (ok.float(), {}), (ok[0], {}), (torch.zeros(2, 2, 8, 8, dtype=torch.uint8), {}),
                       (torch.zeros(2, 0, 8, dtype=torch.uint8), {}), (torch.zeros(2, 129, 8, dtype=torch.uint8), {}),
                       (torch.zeros(2, 8, 6, dtype=torch.uint8), {}), (torch.zeros(2, 8, 132, dtype=torch.uint8), {}),
                       (torch.zeros(2, 8, 0, dtype=torch.uint8), {}), (ok, dict(threshold=0)), (ok, dict(threshold=256)),
                       (ok, dict(threshold=1.5)), (ok, dict(connectivity=6)), (ok, dict(connectivity=True)), (ok, dict(min_area=0)),
                       (ok, dict(min_area="4"))]:
        with pytest.raises(ValueError):
            components.component_stats(images, **kw)
    for kw in (dict(fill=127), dict(fill=256), dict(threshold=200, fill=199)):
        with pytest.raises(ValueError, match="fill"):
            components.despeckle_u8(ok, **kw)
    for fn in (components.component_stats, components.component_roots, components.despeckle_u8):
        with pytest.raises(ValueError, match="no CPU path"):                   # every argument fine but the device
            fn(ok)
    with pytest.raises(ValueError, match="contiguous|no CPU path"):
        components.component_stats(torch.zeros(2, 8, 16, dtype=torch.uint8)[:, :, ::2])


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)                                                 # host memory: a refused call reads none of it
    p = C.c_void_p(buf.ctypes.data)
    call = lambda **k: lib.siggan_components_u8(0, k.get("u8", p), k.get("batch", 1), k.get("h", 4), k.get("w", 4), k.get("thr", 128),   # noqa: E731
                                                k.get("conn", 8), k.get("min_area", 1), k.get("fill", 255), k.get("stats", p), None, None, None)
    for bad in (dict(batch=0), dict(h=0), dict(h=129), dict(w=2), dict(w=10), dict(w=132), dict(thr=0), dict(thr=256), dict(conn=5),
                dict(min_area=0), dict(fill=127), dict(fill=256), dict(stats=None), dict(u8=None), dict(u8=C.c_void_p(buf.ctypes.data + 2))):
        assert call(**bad) == _lib.E_ARG, bad
        assert lib.siggan_last_error()


def test_exports_are_listed():
    assert _lib.COMPONENTS_EXPORTS == ("siggan_components_u8",)
    assert hasattr(_lib.load(), "siggan_components_u8")
    assert _lib.CC_COUNT == 9 == len(components.STAT_NAMES) and _lib.CC_MAX_SIZE == 128
    assert _lib.ABI_VERSION == 4 and _lib.load().siggan_abi_version() == 4
    assert (components.INK, components.COMPONENTS, components.Y1) == (CC.INK, CC.COMPONENTS, CC.Y1) == (0, 1, 8)


def test_both_clis_parse_the_new_flags_and_keep_their_defaults():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import generate_signatures as gen
    base = ["--checkpoint", "x.pth"]
    a = ev.parse_args(base)
    assert a.components is None and "components" not in vars(a)                  # a command line without it parses to what it did
    assert ev.parse_args(base + ["--components"]).components == "auto"
    assert ev.parse_args(base + ["--components", "9"]).components == 9
    with pytest.raises(SystemExit):
        ev.parse_args(base + ["--components", "0"])
    g = gen.parse_args(base)
    assert "despeckle" not in vars(g) and gen.despeckle_opt(g) is None and gen.with_despeckle(None) == {}
    d = gen.despeckle_opt(gen.parse_args(base + ["--despeckle"]))
    assert d.report() == {"min_area": None, "threshold": 128, "connectivity": 8, "removed_components": 0, "removed_pixels": 0}
    d = gen.despeckle_opt(gen.parse_args(base + ["--despeckle", "7", "--threshold", "100", "--filter_by_realism"]))
    assert (d.min_area, d.threshold) == (7, 100)
    for bad in (["--despeckle", "0"], ["--despeckle", "--project", "p"], ["--despeckle", "--morph"], ["--despeckle", "--threshold", "0"]):
        with pytest.raises(SystemExit):
            gen.parse_args(base + bad)
    assert gen.records_json([1, 2], None) == [1, 2] and set(gen.records_json([1], d)) == {"despeckle", "records"}
    d.count(np.array([[9, 3, 5, 2, 4, 0, 0, 1, 1], [0, 0, 0, 0, 0, -1, -1, -1, -1]]))
    assert (d.removed_components, d.removed_pixels) == (2, 4)
    # the summary prints its fragmentation lines only when the key is there
    import contextlib
    import io
    out = io.StringIO()
    m = {"n_samples": 1, "image_shape": [1, 64, 64]}
    with contextlib.redirect_stdout(out):
        ev.print_summary(m)
    assert "Fragmentation" not in out.getvalue()
    frag = metrics.fragmentation_from_counters(np.array([[9, 3, 5, 2, 4, 0, 0, 1, 1]]))
    with contextlib.redirect_stdout(out):
        ev.print_summary(dict(m, fragmentation={"generated": frag, "threshold": 128, "connectivity": 8, "min_area": 4}))
    assert "Fragmentation" in out.getvalue() and "Generated: 3.00 components" in out.getvalue()
