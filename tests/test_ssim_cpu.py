"""SSIM without a device: the float64 restatement against closed forms and an independent scipy formulation, the window the
library hands out, the numpy reductions on hand-made matrices, the refusals and the two CLIs' new flags
(tests/ssimcommon.py, signature_gan_amd/ssim.py, include/siggan_ssim.h)."""
import contextlib
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import ssimcommon as SC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, ssim
from signature_gan_amd.utils import metrics

SHAPES = [(11, 12), (16, 16), (40, 52), (64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_restatement_gives_one_for_an_image_against_itself_and_is_symmetric(shape):
    a, b = SC.image_lists(*shape, 10, 9)
    aa, ab, ba = SC.ssim_matrix64(a, a), SC.ssim_matrix64(a, b), SC.ssim_matrix64(b, a)
    assert np.array_equal(np.diag(aa), np.ones(len(a)))               # exactly: numerator and denominator are the same numbers
    assert np.array_equal(ab, ba.T) and np.array_equal(aa, aa.T)
    assert ab[0, 1] == ab[0, 7] == 1.0 and ab[1, 2] == 1.0 and ab[2, 3] == 1.0 and ab[4, 6] == 1.0    # the planted duplicates
    assert (ab <= 1.0).all() and (ab >= -1.0).all() and ab.min() < 0.5
    assert SC.ssim64(a[0], a[6]) < 1.0                                # the shifted copy is not the image


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_constant_images_have_the_closed_form(shape):
    h, w = shape
    # The float-rounded taps do not sum to 1 exactly: the window's weight is S = (sum g)^2 = 1 + d with |d| ~ 1e-8.  Then
    # mu = a S, var_a = a^2 S (1 - S), cov = a b S (1 - S): the contrast term is 1 - (a - b)^2 S d / (...+ C2) instead of 1, and
    # the luminance term moves by less than 4 |d|.  The closed form holds up to that.
    d = abs(float(SC.taps().astype(np.float64).sum()) ** 2 - 1.0)
    assert d < 1e-7
    for va, vb in ((255, 0), (255, 255), (0, 0), (10, 200), (128, 127)):
        x, y = np.full((h, w), va, np.uint8), np.full((h, w), vb, np.uint8)
        want = (2.0 * va * vb + SC.C1) / (va * va + vb * vb + SC.C1)  # both variances and the covariance vanish
        assert abs(SC.ssim64(x, y) - want) <= ((va - vb) ** 2 / SC.C2 + 4.0) * d + 1e-12, (va, vb)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_restatement_agrees_with_scipys_correlate1d(shape):
    a, b = SC.image_lists(*shape, 10, 9)
    m = SC.ssim_matrix64(a, b)
    for i, j in ((0, 0), (0, 4), (3, 0), (4, 5), (6, 1), (1, 3), (9, 8)):
        assert abs(SC.ssim_scipy(a[i], b[j]) - m[i, j]) <= 1e-12, (i, j)
    # and the plain-fp32 restatement is fp32-close to it, which is what the GPU bound is scaled by
    dev = np.abs(SC.ssim_matrix32(a, b).astype(np.float64) - m).max()
    assert 0 < dev < 1e-4


def test_the_librarys_window_is_the_numpy_taps():
    g = SC.taps()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.array_equal(ssim.window().view(np.int32), g.view(np.int32))
    assert np.array_equal(g, g[::-1]) and abs(float(g.astype(np.float64).sum()) - 1.0) < 1e-7 and g.argmax() == 5
    assert (ssim.WINDOW_TAPS, ssim.WINDOW_SIGMA) == (SC.TAPS, SC.SIGMA) == (11, 1.5)
    assert _lib.load().siggan_ssim_window(None) == _lib.E_ARG


def test_diversity_on_hand_made_matrices():
    m = np.array([[1.0, 0.5, 0.25], [0.5, 1.0, 0.0], [0.25, 0.0, 1.0]])
    d = ssim.ssim_diversity(m)
    assert d["n"] == 3 and d["all_pairs"] == {"pairs": 3, "mean_ssim": 0.25, "diversity": 0.75} and d["lpips_pairs"] == d["all_pairs"]
    assert ssim.ssim_diversity(torch.tensor(m, dtype=torch.float32)) == d
    # both pair sets differ from 11 images on (j < i + 10) and from 101 on (the first 100 images)
    for n in (11, 12, 100, 101, 130):
        rng = np.random.default_rng(n)
        m = rng.random((n, n))
        m = (m + m.T) / 2
        d = ssim.ssim_diversity(m)
        first = min(100, n)
        near = [m[i, j] for i in range(first) for j in range(i + 1, first) if j < i + 10]
        every = [m[i, j] for i in range(n) for j in range(i + 1, n)]
        assert d["lpips_pairs"]["pairs"] == len(near) and d["all_pairs"]["pairs"] == len(every) == n * (n - 1) // 2
        assert d["lpips_pairs"]["mean_ssim"] == pytest.approx(np.mean(near), abs=1e-12)
        assert d["all_pairs"]["mean_ssim"] == pytest.approx(np.mean(every), abs=1e-12)
        assert d["all_pairs"]["diversity"] == 1.0 - d["all_pairs"]["mean_ssim"]
    assert ssim.ssim_diversity(m)["lpips_pairs"]["pairs"] == sum(min(9, 99 - i) for i in range(100))
    one = ssim.ssim_diversity(np.ones((1, 1)))                                    # n = 1: no pair
    assert one == {"n": 1, "lpips_pairs": {"pairs": 0, "mean_ssim": None, "diversity": None},
                   "all_pairs": {"pairs": 0, "mean_ssim": None, "diversity": None}}
    for bad in (np.ones((2, 3)), np.ones(4), np.ones((0, 0))):
        with pytest.raises(ValueError):
            ssim.ssim_diversity(bad)


def test_nearest_real_on_hand_made_results():
    best = np.array([0.5, 0.9, 0.9, 0.1, 0.7, 0.9, 0.3], np.float32)
    index = np.array([4, 2, 0, 1, 3, 5, 6], np.int32)
    loo = np.array([0.4, 0.6, 0.2, 0.8], np.float32)
    d = ssim.nearest_real_from_best(best, index, loo)
    f = lambda v: float(np.float32(v))                                             # noqa: E731
    assert d["n_generated"] == 7 and d["n_real_loo"] == 4
    assert d["median"] == f(0.7) and d["max"] == f(0.9) and d["mean"] == pytest.approx(float(best.astype(np.float64).mean()))
    assert d["real_loo_median"] == (f(0.4) + f(0.6)) / 2 and d["excess_median"] == d["median"] - d["real_loo_median"] > 0
    # ties in `closest`: by SSIM descending, equal values by generated index
    assert d["closest"] == [(1, 2, f(0.9)), (2, 0, f(0.9)), (5, 5, f(0.9)), (4, 3, f(0.7)), (0, 4, f(0.5))]
    assert ssim.nearest_real_from_best(torch.from_numpy(best), torch.from_numpy(index), torch.from_numpy(loo)) == d
    one = ssim.nearest_real_from_best([0.25], [3])                                 # one generated image, a real set of one
    assert one == {"n_generated": 1, "n_real_loo": 0, "mean": 0.25, "median": 0.25, "max": 0.25, "real_loo_median": None,
                   "excess_median": None, "closest": [(0, 3, 0.25)]}
    assert ssim.nearest_real_from_best([0.25], [3], [])["real_loo_median"] is None
    for bad in (([], []), ([0.1, 0.2], [1])):
        with pytest.raises(ValueError):
            ssim.nearest_real_from_best(*bad)


def test_refusals_that_need_no_device():
    ok = torch.zeros(2, 16, 16, dtype=torch.uint8)
    cases = [(np.zeros((2, 16, 16), np.uint8), "tensor"), (ok.float(), "uint8"), (ok[0], "N, H, W"),
             (torch.zeros(2, 2, 16, 16, dtype=torch.uint8), "N, H, W"), (ok[:0], "no image"),
             (torch.zeros(2, 10, 16, dtype=torch.uint8), "height"), (torch.zeros(2, 129, 16, dtype=torch.uint8), "height"),
             (torch.zeros(2, 16, 8, dtype=torch.uint8), "width"), (torch.zeros(2, 16, 14, dtype=torch.uint8), "width"),
             (torch.zeros(2, 16, 132, dtype=torch.uint8), "width"), (ok, "no CPU path")]
    for images, word in cases:
        for call in (lambda: ssim.SsimSet(images), lambda: ssim.ssim_matrix(images), lambda: ssim.ssim_best(images),
                     lambda: ssim.ssim_paired(images, images), lambda: ssim.ssim_matrix_and_best(images)):
            with pytest.raises(ValueError, match=word):
                call()
    # the order: type, dtype, rank, sizes, device, layout -- an argument wrong in several ways names the first
    with pytest.raises(ValueError, match="uint8"):
        ssim.SsimSet(torch.zeros(16, 16))                                          # dtype before rank
    with pytest.raises(ValueError, match="N, H, W"):
        ssim.SsimSet(torch.zeros(5, 16, dtype=torch.uint8))                        # rank before sizes
    with pytest.raises(ValueError, match="height"):
        ssim.SsimSet(torch.zeros(2, 10, 8, dtype=torch.uint8))                     # height before width
    with pytest.raises(ValueError, match="width"):
        ssim.SsimSet(torch.zeros(2, 16, 20, dtype=torch.uint8)[:, :, :10])         # sizes before device and layout
    with pytest.raises(ValueError, match="no CPU path"):
        ssim.SsimSet(torch.zeros(2, 16, 32, dtype=torch.uint8)[:, :, ::2])         # device before layout
    with pytest.raises(ValueError, match="NoneType"):
        ssim.ssim_paired(ok, None)
    for fn in (metrics.calculate_ssim_diversity, lambda x: metrics.calculate_ssim_nearest_real(x, x)):
        with pytest.raises(ValueError, match="tensor"):
            fn(np.zeros((2, 16, 16), np.uint8))


def test_the_library_refuses_before_it_touches_a_device():
    lib = _lib.load()
    buf = np.zeros(64, np.int32)                                                   # host memory: a refused call reads none of it
    p, odd = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 2)

    def pairs(**k):
        return lib.siggan_ssim_pairs(0, k.get("a_u8", p), k.get("a_maps", p), k.get("na", 2), k.get("b_u8", p), k.get("b_maps", p),
                                     k.get("nb", 2), k.get("h", 16), k.get("w", 16), k.get("mode", _lib.SSIM_ALL),
                                     k.get("matrix", p), k.get("best", None), k.get("index", None), None)
    other = C.c_void_p(buf.ctypes.data + 64)
    for bad in (dict(na=0), dict(nb=0), dict(na=-1), dict(h=10), dict(h=129), dict(w=8), dict(w=14), dict(w=132), dict(mode=-1),
                dict(mode=3), dict(matrix=None), dict(a_u8=None), dict(a_maps=None), dict(b_u8=None), dict(b_maps=None),
                dict(a_u8=odd), dict(a_maps=odd), dict(b_u8=odd), dict(b_maps=odd), dict(matrix=odd), dict(best=odd),
                dict(index=odd), dict(mode=_lib.SSIM_PAIRED, nb=3), dict(mode=_lib.SSIM_PAIRED, best=p),
                dict(mode=_lib.SSIM_PAIRED, index=p), dict(mode=_lib.SSIM_SAME_SET, nb=3), dict(mode=_lib.SSIM_SAME_SET, b_u8=other),
                dict(mode=_lib.SSIM_SAME_SET, b_maps=other)):
        assert pairs(**bad) == _lib.E_ARG, bad
        assert lib.siggan_last_error()
    for n, h, w, u8, maps in ((0, 16, 16, p, p), (1, 10, 16, p, p), (1, 129, 16, p, p), (1, 16, 8, p, p), (1, 16, 18, p, p),
                              (1, 16, 132, p, p), (1, 16, 16, None, p), (1, 16, 16, p, None), (1, 16, 16, odd, p), (1, 16, 16, p, odd)):
        assert lib.siggan_ssim_prepare_u8(0, u8, n, h, w, maps, None) == _lib.E_ARG, (n, h, w)
    assert not buf.any()
    assert lib.siggan_ssim_maps_bytes(3, 64, 64) == 3 * 2 * 54 * 54 * 4 and lib.siggan_ssim_maps_bytes(1, 11, 12) == 2 * 1 * 2 * 4
    assert lib.siggan_ssim_maps_bytes(0, 64, 64) == _lib.E_ARG and lib.siggan_ssim_maps_bytes(1, 64, 130) == _lib.E_ARG


def test_the_split_planner_is_the_two_planners_it_replaced(tmp_path):
    """csrc/pair_plan.h -- how siggan_ssim_pairs and siggan_dtw_pairs split b's columns over the grid -- against the two
    formulas it replaced and against what the kernels need of a plan (1 <= S <= 32, whole units per split, no empty split,
    every column owned), for every nb in 1..4096, 44 values of row_tiles and unit in 1..8, by the stand-alone
    csrc/pair_plan_check.cpp under AddressSanitizer and UBSan: this is what the test is about, so it starts the compiler and
    the program."""
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "signature-gan_amd", "csrc")
    exe = str(tmp_path / "pair_plan_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(csrc, "pair_plan_check.cpp")],
                   check=True, cwd=str(tmp_path))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == f"OK {4096 * 44 * 8}", run.stdout + run.stderr


def test_exports_match_the_header():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "siggan_ssim.h")).read()
    declared = re.findall(r"^(?:int|int64_t) (siggan_\w+)\(", header, flags=re.M)
    assert tuple(declared) == _lib.SSIM_EXPORTS == ("siggan_ssim_window", "siggan_ssim_maps_bytes", "siggan_ssim_prepare_u8",
                                                    "siggan_ssim_pairs")
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in _lib.SSIM_EXPORTS)
    assert not set(_lib.SSIM_EXPORTS) & set(_lib.EXPORTS)
    assert _lib.ABI_VERSION == 4 and lib.siggan_abi_version() == 4
    define = lambda name: re.search(rf"#define {name} (\S+)", header).group(1)     # noqa: E731
    assert (int(define("SIGGAN_SSIM_TAPS")), float(define("SIGGAN_SSIM_SIGMA")), int(define("SIGGAN_SSIM_MIN_HEIGHT")),
            int(define("SIGGAN_SSIM_MIN_WIDTH")), int(define("SIGGAN_SSIM_MAX_SIZE"))) == (
        _lib.SSIM_TAPS, _lib.SSIM_SIGMA, _lib.SSIM_MIN_HEIGHT, _lib.SSIM_MIN_WIDTH, _lib.SSIM_MAX_SIZE)
    enum = re.search(r"enum \{([^}]*)\}", header).group(1)
    assert re.findall(r"SIGGAN_SSIM_\w+", enum) == ["SIGGAN_SSIM_ALL", "SIGGAN_SSIM_SAME_SET", "SIGGAN_SSIM_PAIRED"]
    assert (_lib.SSIM_ALL, _lib.SSIM_SAME_SET, _lib.SSIM_PAIRED) == (0, 1, 2)


def test_both_clis_flags_are_absent_from_the_namespace_unless_given():
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import generate_signatures as gen
    base = ["--checkpoint", "x.pth"]
    a = ev.parse_args(base)
    assert a.ssim is False and "ssim" not in vars(a)
    b = ev.parse_args(base + ["--ssim"])
    assert b.ssim is True and {k: v for k, v in vars(b).items() if k != "ssim"} == vars(a)
    g = gen.parse_args(base + ["--project", "p"])
    assert "project_ssim" not in vars(g) and gen.project_ssim_opt(g) is False
    g2 = gen.parse_args(base + ["--project", "p", "--project_ssim"])
    assert gen.project_ssim_opt(g2) is True and {k: v for k, v in vars(g2).items() if k != "project_ssim"} == vars(g)
    with pytest.raises(SystemExit):
        gen.parse_args(base + ["--project_ssim"])                                  # needs --project
    # the summary prints its SSIM lines only when the key is there, below an unchanged LPIPS line
    m = {"n_samples": 1, "image_shape": [1, 64, 64], "lpips_error": "lpips package not available"}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ev.print_summary(m)
    plain = out.getvalue()
    assert "SSIM" not in plain
    div = ssim.ssim_diversity(np.array([[1.0, 0.25], [0.25, 1.0]]))
    near = ssim.nearest_real_from_best([0.5, 0.75], [1, 0], [0.5, 0.5])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ev.print_summary(dict(m, pixel_similarity={"generated_diversity": div, "real_diversity": div, "nearest_real": near}))
    lines, before = out.getvalue().splitlines(), plain.splitlines()
    at = lines.index("LPIPS Diversity: Not computed - lpips package not available")
    assert lines[at + 1].startswith("SSIM Diversity: 0.7500") and "real set: 0.7500" in lines[at + 1]
    assert lines[at + 2].startswith("SSIM to the nearest real image: median 0.6250, max 0.7500") and "excess 0.1250" in lines[at + 2]
    assert lines[:at + 1] + lines[at + 3:] == before
