"""k-means and mode counting without a device: the binding against include/siggan_kmeans.h, the workspace size, every refusal
of the three calls (argument checks in front of any HIP call, so they run without a GPU), the yardstick (tests/kmeanscommon.py)
on its own, ndb_from_counts on numbers worked by hand, pixel_features against numpy, and every refusal text of utils/modes.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import kmeanscommon as K
import rngcommon as R
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils import modes

HEADER = open(os.path.join(ROOT, "include", "siggan_kmeans.h")).read()
NO_CPU = "a ROCm device ('cuda:N'); there is no CPU path"


# ------------------------------------------------------------------------------------------------------ binding and header
def test_library_exports_the_kmeans_header():
    declared = re.findall(r"\n(?:int|size_t)\s+(siggan_\w+)\s*\(", HEADER)
    assert tuple(declared) == _lib.KMEANS_SYMBOLS == ("siggan_kmeans_workspace", "siggan_kmeans_seed", "siggan_kmeans_lloyd")
    assert _lib._KMEANS_SIGNATURES in _lib.ADDED_GROUPS and set(declared) <= set(_lib.ADDED_SYMBOLS)
    lib = _lib.load()
    for name in declared:
        assert hasattr(C.CDLL(_lib.LIB_PATH), name), f"{name} declared in siggan_kmeans.h but not exported"
        proto = re.search(rf"{name}\((.*?)\);", HEADER, re.S).group(1)
        assert len(proto.split(",")) == len(_lib._KMEANS_SIGNATURES[name][1]) == len(getattr(lib, name).argtypes)
    assert lib.siggan_abi_version() == 4                                             # symbols only added


def test_none_of_them_is_in_the_core_symbol_set():
    with open(os.path.join(ROOT, "include", "siggan.h")) as f:
        core = f.read()
    assert not set(_lib.KMEANS_SYMBOLS) & set(_lib.EXPORTS) and not set(_lib.KMEANS_SYMBOLS) & set(_lib.ALL_EXPORTS + _lib.EXTRA_SYMBOLS)
    assert "siggan_kmeans" not in core
    assert len(_lib.EXPORTS) == 64 and _lib.EXPORTS[-1] == "mlpgan_op_gemm"


def test_the_constants_agree_with_the_header():
    define = lambda name: re.search(rf"#define SIGGAN_KMEANS_{name}\s+(\S+)", HEADER).group(1)     # noqa: E731
    assert int(define("MAX_N")) == _lib.KMEANS_MAX_N == _lib.DIVERSE_MAX_N
    assert int(define("MAX_DIM")) == _lib.KMEANS_MAX_DIM == _lib.KNN_MAX_DIM
    assert int(define("MAX_K")) == _lib.KMEANS_MAX_K == 256
    assert int(define("MAX_ITERATIONS")) == _lib.KMEANS_MAX_ITERATIONS == 1000
    assert int(define("SUM_BLOCK")) == _lib.KMEANS_SUM_BLOCK == K.SUM_BLOCK == 64
    assert int(define("FEATURE_SLAB")) == _lib.KMEANS_FEATURE_SLAB == 256
    assert int(define("STREAM").rstrip("u"), 16) == _lib.KMEANS_STREAM == K.SID_KMEANS == int.from_bytes(b"KMPP", "big")
    others = [R.SID_Z, R.SID_ZG, R.SID_RANDN, R.SID_FC1, R.SID_FC2, R.SID_CLS, _lib.WARP_STREAM] + [R.SID_DROP0 + l for l in range(17)]
    assert K.SID_KMEANS not in others, "the seeding's stream id is its own"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "0x4B4D5050" in design, "DESIGN.md 3, Random streams, lists the stream"


def test_workspace_size():
    lib = _lib.load()
    ws = lib.siggan_kmeans_workspace
    for n, dim, k in ((0, 4, 1), (-1, 4, 1), (_lib.KMEANS_MAX_N + 1, 4, 1), (8, 0, 1), (8, _lib.KMEANS_MAX_DIM + 1, 1), (8, 4, 0),
                      (8, 4, 9), (1000, 4, _lib.KMEANS_MAX_K + 1), (1, 1, 2)):
        assert ws(n, dim, k) == 0, (n, dim, k)
    assert ws(1, 1, 1) > 0 and ws(_lib.KMEANS_MAX_N, _lib.KMEANS_MAX_DIM, _lib.KMEANS_MAX_K) > 0
    by_n = [ws(n, 40, 1) for n in (1, 63, 64, 65, 257, 1031, 4099, _lib.KMEANS_MAX_N)]
    by_dim = [ws(1031, dim, 16) for dim in (1, 4, 5, 257, 1024)]
    by_k = [ws(1031, 40, k) for k in (1, 2, 17, 256)]
    for sizes in (by_n, by_dim, by_k):
        assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes), sizes
    assert by_n[-1] >= 12 * _lib.KMEANS_MAX_N                                        # fp64 values and last pass's labels at the least


def test_every_refusal_comes_before_any_device_call():
    """Host memory stands in for every pointer: a refused call dereferences none and launches nothing."""
    lib = _lib.load()
    n, dim, k = 8, 4, 3
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    size = lib.siggan_kmeans_workspace(n, dim, k)
    assert 0 < size <= 4096 * 8

    def seed(x=ptr, n=n, dim=dim, k=k, centres=ptr, rows=ptr, ws=ptr, ws_bytes=size):
        return lib.siggan_kmeans_seed(0, x, n, dim, k, 5, centres, rows, ws, ws_bytes, None)

    def lloyd(x=ptr, n=n, dim=dim, centres=ptr, k=k, iterations=2, label=ptr, count=ptr, inertia=ptr, changed=ptr, ws=ptr, ws_bytes=size):
        return lib.siggan_kmeans_lloyd(0, x, n, dim, centres, k, iterations, label, None, count, inertia, changed, ws, ws_bytes, None)

    sizes = [dict(n=0), dict(n=-3), dict(n=_lib.KMEANS_MAX_N + 1, ws_bytes=1 << 30), dict(dim=0), dict(dim=_lib.KMEANS_MAX_DIM + 1),
             dict(k=0), dict(k=-1), dict(k=n + 1), dict(k=_lib.KMEANS_MAX_K + 1, n=1000, ws_bytes=1 << 30), dict(x=None),
             dict(centres=None), dict(ws=None), dict(ws_bytes=size - 1), dict(ws_bytes=0), dict(ws=C.c_void_p(ptr.value + 4))]
    for call, more in ((seed, [dict(rows=None)]),
                       (lloyd, [dict(label=None), dict(count=None), dict(inertia=None), dict(changed=None), dict(iterations=-1),
                                dict(iterations=_lib.KMEANS_MAX_ITERATIONS + 1)])):
        for kw in sizes + more:
            assert call(**kw) == _lib.E_ARG, (call.__name__, kw)
            assert lib.siggan_last_error(), kw
        assert call(x=None) == _lib.E_ARG and b"null" in lib.siggan_last_error()
        assert call(ws_bytes=size - 1) == _lib.E_ARG and b"workspace" in lib.siggan_last_error()
        assert call(k=n + 1) == _lib.E_ARG and b"exceeds" in lib.siggan_last_error()
        assert call(ws=C.c_void_p(ptr.value + 4)) == _lib.E_ARG and b"aligned" in lib.siggan_last_error()
    assert lloyd(iterations=1001) == _lib.E_ARG and b"iterations" in lib.siggan_last_error()


# ------------------------------------------------------------------------------------------------------------ the yardstick
def test_two_level_sum_is_the_header_s():
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 128, 129, 1031):
        v = rng.random(n) ** 4
        total, prefix = K.two_level(v)
        slow_total, slow_prefix = K.two_level_slow(v)
        assert total == slow_total and np.array_equal(prefix, slow_prefix), n
        assert prefix[-1] == total and np.all(np.diff(prefix) >= 0)
    v = rng.random(1031)
    assert K.two_level(v)[0] != float(np.cumsum(v)[-1]) or K.two_level(v)[0] != float(v.sum()), "the order is part of the value"


def test_uniform_is_in_range_and_exact():
    for seed in (0, 7, (1 << 32) + 7):
        for s in range(40):
            u = K.uniform(seed, s)
            assert 0.0 <= u < 1.0 and u * 2.0 ** 53 == int(u * 2.0 ** 53)
    assert K.uniform(0, 1) != K.uniform(1 << 32, 1), "the seed's high half is keyed"
    assert K.uniform(3, 1) != K.uniform(3, 2)


def test_seeding_rule_and_its_fallbacks():
    x = K.normal(5, 257)
    rows, steps = K.seed_rows(x, 17, 0)
    assert len(set(rows.tolist())) == 17 and all(st["rule"] == "prefix" for st in steps[1:])
    assert rows[0] == min(256, int(K.uniform(0, 0) * 257))
    # fewer distinct rows than k: once every distinct row is chosen T == 0 and the lowest rows not chosen follow, ascending
    base = K.lattice(4, 3)
    assert len({r.tobytes() for r in base}) == 3
    dup = np.repeat(base, 4, axis=0)                                                 # 12 rows, 3 distinct
    rows, steps = K.seed_rows(dup, 8, 5)
    assert len(set(rows.tolist())) == 8
    assert len({dup[r].tobytes() for r in rows[:3]}) == 3 and [st["rule"] for st in steps[3:]] == ["unchosen"] * 5
    rest = [r for r in range(12) if r not in set(rows[:3].tolist())]
    assert rows[3:].tolist() == rest[:5]
    # a chosen row carries no weight: it is never drawn again while T > 0
    for seed in range(6):
        rows, _ = K.seed_rows(K.lattice(3, 40, seed), 20, seed)
        assert len(set(rows.tolist())) == 20


def test_lloyd_pass_agrees_with_brute_force():
    for dim, n, k in ((1, 17, 2), (5, 257, 16), (40, 67, 17)):
        x, c = K.normal(dim, n), K.normal(dim, n + 1)[:k]
        labels, mind2, undecided, _ = K.assign(x, c)
        x64, c64 = x.astype(np.float64), c.astype(np.float64)
        for i in range(n):
            d = [math.fsum((a - b) ** 2 for a, b in zip(x64[i], cj)) for cj in c64]
            j = min(range(k), key=lambda j: (d[j], j))
            assert undecided[i] or j == labels[i]
            assert abs(d[labels[i]] - mind2[i]) <= (dim + 4) * K.EPS * max(d[labels[i]], 1e-300)
        assert not undecided.any()
        centres, counts = K.update(x, labels, c)
        assert counts.sum() == n
        for j in range(k):
            rows = np.flatnonzero(labels == j)
            if rows.size == 0:
                assert centres[j].tobytes() == c[j].tobytes()
                continue
            for f in range(dim):
                s = 0.0
                for i in rows:
                    s = s + float(x64[i, f])
                assert centres[j, f] == np.float32(s / rows.size)
    ties = K.lattice(2, 65)
    labels, mind2, undecided, _ = K.assign(ties, np.concatenate([ties[:4], ties[:4]]))
    assert labels.max() < 4 and not undecided.any(), "equal distances go to the lower centre, and exact ones are decided"


def test_blobs_are_separated_and_unequal():
    x, blob = K.blobs(5, 257, 3)
    sizes = np.bincount(blob, minlength=3)
    assert sizes.sum() == 257 and sizes[0] < sizes[1] < sizes[2]
    means = np.stack([x[blob == j].mean(0) for j in range(3)])
    labels, _, undecided, _ = K.assign(x, means.astype(np.float32))
    assert np.array_equal(labels, blob) and not undecided.any()


# ------------------------------------------------------------------------------------------------------- ndb_from_counts
def test_ndb_on_three_bins_by_hand():
    # r = (50, 30, 20), t = (50, 30, 20): equal proportions
    same = modes.ndb_from_counts([50, 30, 20], [100, 60, 40])
    assert same["ndb"] == 0 and same["js_divergence"] == 0.0 and same["z"] == [0.0, 0.0, 0.0] and same["missing_bins"] == []
    assert same["most_under_represented"] == [] and (same["k"], same["n_ref"], same["n_test"]) == (3, 100, 200)
    # r = (50, 50, 0), t = (50, 0, 50), N = 100 each.  Bin 0: p = q: z = 0.  Bin 1: p = .5, q = 0, P = .25:
    # z = .5 / sqrt(.25 * .75 * .02) = .5 / sqrt(.00375).  Bin 2: the mirror image.
    d = modes.ndb_from_counts([50, 50, 0], [50, 0, 50])
    z1 = 0.5 / math.sqrt(0.25 * 0.75 * 0.02)
    assert d["z"][0] == 0.0 and d["z"][1] == pytest.approx(z1, rel=1e-14) and d["z"][2] == pytest.approx(-z1, rel=1e-14)
    assert d["different_bins"] == [1, 2] and d["ndb"] == 2 and d["ndb_over_k"] == pytest.approx(2 / 3)
    assert d["missing_bins"] == [1], "bin 2 is empty in the reference: nothing is missing there"
    assert d["most_under_represented"] == [[1, d["z"][1], 50, 0]]
    # JS by hand: p = (.5, .5, 0), q = (.5, 0, .5), mid = (.5, .25, .25): KL(p|mid) = .5 log2(2) = .5 = KL(q|mid): JS = .5
    assert d["js_divergence"] == pytest.approx(0.5, abs=1e-15)
    # a bin empty on both sides: the denominator is 0 and z is 0 by definition
    e = modes.ndb_from_counts([10, 0, 10], [12, 0, 8])
    assert e["z"][1] == 0.0 and e["ndb"] == 0 and e["missing_bins"] == []
    # everything in one bin on both sides: P = 1 there, the denominator is 0 everywhere
    assert modes.ndb_from_counts([7, 0], [9, 0])["z"] == [0.0, 0.0]
    # the threshold is the two-sided normal one: |z| = 1.96 is at p = 0.05
    assert math.erfc(1.959963984540054 / math.sqrt(2)) == pytest.approx(0.05, rel=1e-12)
    # alpha moves the count: r = (60, 40), t = (50, 50), N = 100: z = .1 / sqrt(.55 * .45 * .02) = 1.421: p = .155
    assert modes.ndb_from_counts([60, 40], [50, 50])["ndb"] == 0 and modes.ndb_from_counts([60, 40], [50, 50], alpha=0.2)["ndb"] == 2


def test_js_divergence_ends_and_symmetry():
    assert modes.ndb_from_counts([5, 5, 0, 0], [0, 0, 3, 7])["js_divergence"] == 1.0
    assert modes.ndb_from_counts([5, 9, 1], [10, 18, 2])["js_divergence"] == 0.0
    rng = np.random.default_rng(11)
    for _ in range(20):
        r, t = rng.integers(0, 30, 12), rng.integers(0, 30, 12)
        r[0] += 1
        t[0] += 1
        a, b = modes.ndb_from_counts(r, t), modes.ndb_from_counts(t, r)
        assert a["js_divergence"] == pytest.approx(b["js_divergence"], abs=1e-15) and 0.0 <= a["js_divergence"] <= 1.0
        assert np.allclose(a["z"], -np.asarray(b["z"]), rtol=0, atol=1e-12) and a["ndb"] == b["ndb"]
    five = modes.ndb_from_counts([10] * 8, [1, 2, 3, 4, 5, 6, 7, 52])["most_under_represented"]
    assert [row[0] for row in five] == [0, 1, 2, 3, 4] and all(row[1] > 0 for row in five)


def test_ndb_refusals():
    for args, text in ((([1, 2], [1, 2, 3]), "same K"), (([], []), "same K"), (([1, -1], [1, 1]), "non-negative"),
                       (([1.5, 1], [1, 1]), "non-negative integers"), (([0, 0], [1, 1]), "must hold a sample"),
                       (([1, 1], [0, 0]), "must hold a sample")):
        with pytest.raises(ValueError, match=text):
            modes.ndb_from_counts(*args)
    for alpha in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            modes.ndb_from_counts([1, 1], [1, 1], alpha=alpha)


# -------------------------------------------------------------------------------------------------------- pixel_features
def test_pixel_features_against_numpy():
    rng = np.random.default_rng(4)
    for side, factor in ((64, 4), (128, 4), (8, 4), (8, 2), (4, 1)):
        u8 = rng.integers(0, 256, (3, side, side), dtype=np.uint8)
        cells = side // factor
        want = u8.reshape(3, cells, factor, cells, factor).astype(np.float64).mean(axis=(2, 4)).reshape(3, cells * cells)
        got = modes.pixel_features(torch.from_numpy(u8), factor)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, cells * cells) and got.is_contiguous()
        assert np.array_equal(got.numpy().astype(np.float64), want), "a mean of 16 bytes is exact in fp32"
        assert torch.equal(modes.pixel_features(torch.from_numpy(u8)[:, None], factor), got)
    assert modes.pixel_features(torch.zeros(2, 64, 64, dtype=torch.uint8)).shape[1] == 256
    assert modes.pixel_features(torch.zeros(2, 128, 128, dtype=torch.uint8)).shape[1] == 1024
    for bad, text in ((torch.zeros(2, 8, 8), "torch.uint8"), (np.zeros((2, 8, 8), np.uint8), "torch.uint8"),
                      (torch.zeros(2, 8, 12, dtype=torch.uint8), r"\(N, S, S\)"), (torch.zeros(8, 8, dtype=torch.uint8), r"\(N, S, S\)")):
        with pytest.raises(ValueError, match=text):
            modes.pixel_features(bad)
    for factor in (3, 0, 16):
        with pytest.raises(ValueError, match="power of two that divides"):
            modes.pixel_features(torch.zeros(2, 8, 8, dtype=torch.uint8), factor)


# ------------------------------------------------------------------------------------------------------- modes.py refusals
def test_wrappers_refuse_without_a_device():
    rows = torch.zeros(9, 8)
    for call in (lambda: modes.kmeans(rows, 3), lambda: modes.seed_centres(rows, 3), lambda: modes.assign(rows, rows[:2])):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == f"x must be a tensor on {NO_CPU}"
    with pytest.raises(ValueError) as e:
        modes.mode_coverage(rows, rows)
    assert str(e.value) == f"real_feats must be a tensor on {NO_CPU}"
    with pytest.raises(ValueError) as e:
        modes.kmeans([[0.0]], 1)
    assert str(e.value) == f"x must be a tensor on {NO_CPU}"


def test_default_k():
    assert [modes.default_k(n) for n in (1, 39, 40, 60, 1999, 2000, 10 ** 6)] == [2, 2, 2, 3, 99, 100, 100]


def test_the_evaluation_flag(capsys):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    base = ["--checkpoint", "c.pt"]
    assert "modes" not in vars(ev.parse_args(base)) and ev.parse_args(base).modes is None
    assert ev.parse_args(base + ["--real_dir", "r", "--modes"]).modes == "auto"
    assert ev.parse_args(base + ["--real_dir", "r", "--modes", "7"]).modes == 7
    for flags, text in ((["--modes"], "--modes needs --real_dir"), (["--real_dir", "r", "--modes", "1"], r"--modes K must be in [2, 256]"),
                        (["--real_dir", "r", "--modes", "257"], "--modes K must be in [2, 256]")):
        with pytest.raises(SystemExit) as e:
            ev.parse_args(base + flags)
        assert e.value.code == 2 and text in capsys.readouterr().err
