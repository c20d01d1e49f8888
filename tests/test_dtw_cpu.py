"""Elastic signature matching without a device: the numpy restatement's own properties, the header against the binding, the
numpy reductions on hand-made inputs, the refusals and the two CLIs' new flags (tests/dtwcommon.py, signature_gan_amd/dtw.py,
include/siggan_dtw.h)."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import dtwcommon as DC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, dtw
from signature_gan_amd.utils import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_the_header_and_the_makefile_lists_the_source():
    header = open(os.path.join(ROOT, "include", "siggan_dtw.h")).read()
    declared = re.findall(r"^int (siggan_\w+)\(", header, flags=re.M)
    assert tuple(declared) == _lib.DTW_EXPORTS == ("siggan_dtw_profiles_u8", "siggan_dtw_pairs")
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.DTW_EXPORTS)
    assert not set(_lib.DTW_EXPORTS) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 64
    assert _lib._DTW_SIGNATURES in _lib.GROUPS and all(getattr(lib, name).argtypes is not None for name in _lib.DTW_EXPORTS)   # load() bound them
    assert _lib.ABI_VERSION == 4 and lib.siggan_abi_version() == 4
    assert int(re.search(r"#define SIGGAN_DTW_MAX_SIZE (\S+)", header).group(1)) == _lib.DTW_MAX_SIZE == 128
    enum = re.search(r"enum \{([^}]*)\}", header).group(1)
    assert re.findall(r"SIGGAN_DTW_\w+", enum) == ["SIGGAN_DTW_ALL", "SIGGAN_DTW_SAME_SET", "SIGGAN_DTW_PAIRED"]
    assert (_lib.DTW_ALL, _lib.DTW_SAME_SET, _lib.DTW_PAIRED) == (0, 1, 2)
    makefile = open(os.path.join(ROOT, "signature-gan_amd", "csrc", "Makefile")).read()
    assert "dtw.hip" in re.search(r"^SRC = (.*)$", makefile, flags=re.M).group(1).split()
    assert "siggan_dtw" not in open(os.path.join(ROOT, "include", "siggan.h")).read()


def test_the_restatements_profiles_on_a_hand_made_image():
    img = np.full((6, 4), 255, np.uint8)
    img[1, 0] = img[2, 0] = img[4, 0] = 0                                          # two runs, rows 1..4
    img[:, 2] = 0                                                                  # a full column
    img[5, 3] = 127                                                                # one pixel in the last row, just ink
    p = DC.profiles(img[None])[0]
    assert p.tolist() == [[3, 1, 4, 2], [0, 3, 3, 0], [6, 0, 5, 1], [1, 5, 5, 1]]
    assert DC.packed(p[None])[0].tolist() == [3 | 1 << 8 | 4 << 16 | 2 << 24, 3 << 8 | 3 << 16, 6 | 5 << 16 | 1 << 24,
                                              1 | 5 << 8 | 5 << 16 | 1 << 24]
    assert DC.profiles(img[None], threshold=127)[0, 3].tolist() == [0, 3, 3, 0]    # 127 is paper at threshold 127
    rows = np.full((128, 4), 255, np.uint8)
    rows[0::2] = 0
    assert DC.profiles(rows[None])[0, 0].tolist() == [64, 0, 126, 64]              # r reaches ceil(h / 2)


@pytest.mark.parametrize("size", [(7, 12), (64, 64), (33, 68)], ids=lambda s: "x".join(map(str, s)))
def test_the_restatements_own_properties(size):
    w = size[1]
    W = DC.world(*size)
    pa, pb = W.pa, W.pb[:9]
    previous = None
    for band in DC.bands(w):
        aa, ab, ba = DC.dtw_matrix(pa, pa, band), DC.dtw_matrix(pa, pb, band), DC.dtw_matrix(pb, pa, band)
        assert not np.diag(aa).any() and np.array_equal(aa, aa.T) and np.array_equal(ab, ba.T)
        assert ab[0, 1] == ab[0, 4] == 0 and ab[1, 2] == 0 and ab[2, 3] == 0       # the planted duplicates
        assert ab.max() <= w * 446
        if band == 0:
            aligned = DC.local_cost(pa, pb)[:, :, np.arange(w), np.arange(w)].sum(axis=-1)
            assert np.array_equal(ab, aligned)
        if previous is not None:
            assert (ab <= previous).all()                                          # a larger band never increases the distance
        previous = ab
        for i, j in ((0, 0), (3, 5), (4, 8)):
            assert DC.dtw_plain(pa[i], pb[j], band) == ab[i, j], (band, i, j)      # the sweep against the plain double loop
    assert previous.min() == 0 and (DC.dtw_matrix(pa, pb, 0) > previous).any()     # and somewhere it decreases it


def test_the_extremes_do_not_fit_sixteen_bits():
    p = DC.profiles(DC.extreme_images())
    assert p[0, 0].tolist() == [128, 0, 127, 1] and p[1, 0].tolist() == [0, 64, 64, 0] and p[2, 0].tolist() == [64, 0, 126, 64]
    for band in (0, 16, 127):
        assert np.array_equal(DC.dtw_matrix(p, p, band), DC.EXTREMES)
    assert DC.EXTREMES.max() == 32768 > np.iinfo(np.int16).max


def test_a_shifted_copy_is_found_only_with_a_band():
    originals = DC.signature_family(64, 64, 12)
    moved = DC.shifted(originals, 3)
    assert np.array_equal(moved[:, :, 3:], originals[:, :, :-3]) and (moved[:, :, :3] == 255).all() and (originals[:, :, -3:] == 255).all()
    po, pm = DC.profiles(originals), DC.profiles(moved)
    elastic, rigid = DC.dtw_matrix(pm, po, 8), DC.dtw_matrix(pm, po, 0)
    assert np.array_equal(DC.first_minimum(elastic)[1], np.arange(12))             # every moved copy finds its original
    assert (DC.first_minimum(rigid)[1] == np.arange(12)).sum() < 6                 # column against column most of them do not


def test_default_band():
    assert [dtw.default_band(w) for w in (4, 8, 12, 64, 68, 128)] == [1, 1, 1, 8, 8, 16] == [DC.default_band(w) for w in (4, 8, 12, 64, 68, 128)]


def test_diversity_on_hand_made_matrices():
    m = np.array([[0, 8, 4], [8, 0, 24], [4, 24, 0]], np.int32)
    d = dtw.dtw_diversity(m, 4)
    assert d["n"] == 3 and d["w"] == 4 and d["all_pairs"] == {"pairs": 3, "mean_distance": 12.0, "diversity": 3.0}
    assert d["lpips_pairs"] == d["all_pairs"] and dtw.dtw_diversity(torch.from_numpy(m), 4) == d
    for n in (11, 12, 100, 101, 130):
        rng = np.random.default_rng(n)
        m = rng.integers(0, 5000, (n, n))
        m = m + m.T
        d = dtw.dtw_diversity(m, 64)
        first = min(100, n)
        near = [m[i, j] for i in range(first) for j in range(i + 1, first) if j < i + 10]
        every = [m[i, j] for i in range(n) for j in range(i + 1, n)]
        assert d["lpips_pairs"]["pairs"] == len(near) and d["all_pairs"]["pairs"] == len(every) == n * (n - 1) // 2
        assert d["lpips_pairs"]["mean_distance"] == pytest.approx(np.mean(near), abs=1e-9)
        assert d["all_pairs"]["diversity"] == d["all_pairs"]["mean_distance"] / 64 == pytest.approx(np.mean(every) / 64, abs=1e-9)
    one = dtw.dtw_diversity(np.zeros((1, 1), np.int32), 64)                        # a set of one image: no pair
    assert one == {"n": 1, "w": 64, "lpips_pairs": {"pairs": 0, "mean_distance": None, "diversity": None},
                   "all_pairs": {"pairs": 0, "mean_distance": None, "diversity": None}}
    for bad in (np.ones((2, 3)), np.ones(4), np.ones((0, 0))):
        with pytest.raises(ValueError):
            dtw.dtw_diversity(bad, 64)
    with pytest.raises(ValueError):
        dtw.dtw_diversity(m, 0)


def test_nearest_real_on_hand_made_results():
    best = np.array([32, 8, 8, 640, 64, 8, 128], np.int32)
    index = np.array([4, 2, 0, 1, 3, 5, 6], np.int32)
    loo = np.array([64, 96, 32, 128], np.int32)
    d = dtw.nearest_real_from_best(best, index, loo, 8)
    assert d["n_generated"] == 7 and d["n_real_loo"] == 4
    assert d["median"] == 4.0 and d["min"] == 1.0 and d["mean"] == pytest.approx(best.mean() / 8)
    assert d["real_loo_median"] == 10.0 and d["excess_median"] == 6.0              # closer to a real image than they are to each other
    # ties in `closest`: by distance ascending, equal values by generated index
    assert d["closest"] == [(1, 2, 1.0), (2, 0, 1.0), (5, 5, 1.0), (0, 4, 4.0), (4, 3, 8.0)]
    assert dtw.nearest_real_from_best(torch.from_numpy(best), torch.from_numpy(index), torch.from_numpy(loo), 8) == d
    one = dtw.nearest_real_from_best([16], [3], None, 64)                          # one generated image, a real set of one
    assert one == {"n_generated": 1, "n_real_loo": 0, "mean": 0.25, "median": 0.25, "min": 0.25, "real_loo_median": None,
                   "excess_median": None, "closest": [(0, 3, 0.25)]}
    assert dtw.nearest_real_from_best([16], [3], [], 64)["real_loo_median"] is None
    for bad in (([], [], None, 8), ([1, 2], [1], None, 8), ([1], [1], None, 0)):
        with pytest.raises(ValueError):
            dtw.nearest_real_from_best(*bad)


def test_refusals_come_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded for a call that had to be refused")
    monkeypatch.setattr(_lib, "load", no_library)
    u8 = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)                     # noqa: E731
    ok = u8(2, 16, 16)
    cases = [(np.zeros((2, 16, 16), np.uint8), "tensor"), (ok.float(), "uint8"), (ok[0], "N, H, W"), (u8(2, 2, 16, 16), "N, H, W"),
             (ok[:0], "no image"), (u8(2, 0, 16), "height"), (u8(2, 129, 16), "height"), (u8(2, 16, 0), "width"),
             (u8(2, 16, 6), "width"), (u8(2, 16, 132), "width"), (ok, "no CPU path")]
    for images, word in cases:
        for call in (lambda: dtw.DtwSet(images), lambda: dtw.column_profiles(images), lambda: dtw.dtw_matrix(images),
                     lambda: dtw.dtw_best(images), lambda: dtw.dtw_paired(images, images), lambda: dtw.dtw_matrix_and_best(images),
                     lambda: dtw.dtw_matrix(ok, images) if images is not ok else dtw.dtw_matrix(ok, ok)):
            with pytest.raises(ValueError, match=word):
                call()
    # parameters stand between the sizes and the device
    for threshold in (0, 256, 1.5, True):
        for call in (lambda: dtw.DtwSet(ok, threshold), lambda: dtw.column_profiles(ok, threshold)):
            with pytest.raises(ValueError, match="threshold"):
                call()
    for band in (-1, 16, 2.0):
        for call in (lambda: dtw.dtw_matrix(ok, band=band), lambda: dtw.dtw_matrix(ok, ok, band), lambda: dtw.dtw_best(ok, band=band),
                     lambda: dtw.dtw_paired(ok, ok, band), lambda: dtw.dtw_matrix_and_best(ok, ok, band)):
            with pytest.raises(ValueError, match="band"):
                call()
    with pytest.raises(ValueError, match="equally many"):
        dtw.dtw_paired(ok, u8(3, 16, 16))
    for call in (lambda: dtw.dtw_matrix(ok, u8(2, 16, 12)), lambda: dtw.dtw_paired(ok, u8(2, 16, 12)), lambda: dtw.dtw_best(ok, u8(5, 8, 20))):
        with pytest.raises(ValueError, match="equal width"):
            call()
    with pytest.raises(ValueError, match="NoneType"):
        dtw.dtw_paired(ok, None)
    # the order: an argument wrong in several ways names the first
    with pytest.raises(ValueError, match="uint8"):
        dtw.DtwSet(torch.zeros(16, 16))                                            # dtype before rank
    with pytest.raises(ValueError, match="N, H, W"):
        dtw.DtwSet(u8(5, 16))                                                      # rank before sizes
    with pytest.raises(ValueError, match="width"):
        dtw.DtwSet(u8(2, 16, 20)[:, :, :10], 0)                                    # sizes before parameters
    with pytest.raises(ValueError, match="threshold"):
        dtw.DtwSet(u8(2, 16, 32)[:, :, ::2], 0)                                    # parameters before device and layout
    with pytest.raises(ValueError, match="no CPU path"):
        dtw.DtwSet(u8(2, 16, 32)[:, :, ::2])                                       # device before layout
    with pytest.raises(ValueError, match="equal width"):
        dtw.dtw_matrix(ok, u8(2, 16, 12), band=-1)                                 # sizes before the band
    for fn in (metrics.calculate_dtw_diversity, lambda x: metrics.calculate_dtw_nearest_real(x, x)):
        with pytest.raises(ValueError, match="tensor"):
            fn(np.zeros((2, 16, 16), np.uint8))


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)                                                   # host memory: a refused call reads none of it
    p, odd, other = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2), C.c_void_p(buf.ctypes.data + 64)

    def pairs(**k):
        return lib.siggan_dtw_pairs(0, k.get("a", p), k.get("na", 2), k.get("b", p), k.get("nb", 2), k.get("w", 16), k.get("band", 2),
                                    k.get("mode", _lib.DTW_ALL), k.get("matrix", p), k.get("best", None), k.get("index", None), None)
    for bad in (dict(na=0), dict(nb=0), dict(na=-1), dict(w=0), dict(w=6), dict(w=132), dict(band=-1), dict(band=16), dict(mode=-1),
                dict(mode=3), dict(matrix=None), dict(a=None), dict(b=None), dict(a=odd), dict(b=odd), dict(matrix=odd), dict(best=odd),
                dict(index=odd), dict(mode=_lib.DTW_PAIRED, nb=3), dict(mode=_lib.DTW_PAIRED, best=p),
                dict(mode=_lib.DTW_PAIRED, index=p), dict(mode=_lib.DTW_SAME_SET, nb=3), dict(mode=_lib.DTW_SAME_SET, b=other)):
        assert pairs(**bad) == _lib.E_ARG, bad
        assert lib.siggan_last_error()
    for n, h, w, thr, u8, prof in ((0, 16, 16, 128, p, p), (1, 0, 16, 128, p, p), (1, 129, 16, 128, p, p), (1, 16, 0, 128, p, p),
                                   (1, 16, 18, 128, p, p), (1, 16, 132, 128, p, p), (1, 16, 16, 0, p, p), (1, 16, 16, 256, p, p),
                                   (1, 16, 16, 128, None, p), (1, 16, 16, 128, p, None), (1, 16, 16, 128, odd, p), (1, 16, 16, 128, p, odd)):
        assert lib.siggan_dtw_profiles_u8(0, u8, n, h, w, thr, prof, None) == _lib.E_ARG, (n, h, w, thr)
    assert not buf.any()


def test_both_clis_flags_are_opt_in():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import signature_verifier_eval as sv
    base = ["--checkpoint", "x.pth"]
    a = ev.parse_args(base)
    assert a.dtw is None and "dtw" not in vars(a)
    b = ev.parse_args(base + ["--dtw"])
    assert b.dtw == "auto" and {k: v for k, v in vars(b).items() if k != "dtw"} == vars(a)
    assert ev.parse_args(base + ["--dtw", "4"]).dtw == 4 and ev.parse_args(base + ["--dtw", "0"]).dtw == 0
    with pytest.raises(SystemExit):
        ev.parse_args(base + ["--dtw", "-1"])
    base = ["--baseline_model", "m.pth", "--test_dir", "t"]
    a = sv.parse_args(base)
    assert a.dtw_baseline is None
    b = sv.parse_args(base + ["--dtw_baseline"])
    assert b.dtw_baseline == "auto" and {k: v for k, v in vars(b).items() if k != "dtw_baseline"} == \
        {k: v for k, v in vars(a).items() if k != "dtw_baseline"}
    assert sv.parse_args(base + ["--dtw_baseline", "4"]).dtw_baseline == 4
    with pytest.raises(SystemExit):
        sv.parse_args(base + ["--dtw_baseline", "-2"])
    # the summary prints its two DTW lines only when the key is there, below an unchanged LPIPS line
    m = {"n_samples": 1, "image_shape": [1, 64, 64], "lpips_error": "lpips package not available"}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ev.print_summary(m)
    plain = out.getvalue()
    assert "DTW" not in plain
    div = dtw.dtw_diversity(np.array([[0, 96], [96, 0]]), 64)
    near = dtw.nearest_real_from_best([64, 32], [1, 0], [128, 128], 64)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ev.print_summary(dict(m, elastic_similarity={"band": 8, "threshold": 128, "generated_diversity": div, "real_diversity": div,
                                                     "nearest_real": near}))
    lines, before = out.getvalue().splitlines(), plain.splitlines()
    at = lines.index("LPIPS Diversity: Not computed - lpips package not available")
    assert lines[at + 1].startswith("DTW Diversity: 1.5000") and "band 8" in lines[at + 1] and "real set: 1.5000" in lines[at + 1]
    assert lines[at + 2].startswith("DTW to the nearest real image: median 0.7500, min 0.5000") and "excess 1.2500" in lines[at + 2]
    assert lines[:at + 1] + lines[at + 3:] == before
    # the baseline's three numbers on a hand-made case: distances that separate the classes perfectly
    s = sv.dtw_scores(np.array([1, 1, 0, 0]), np.array([10, 20, 30, 40]))
    assert s["auc"] == 1.0 and s["eer"] == 0.0 and s["eer_distance"] == 20.0
