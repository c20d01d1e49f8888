"""CPU-only checks of diverse selection: the yardstick (diversecommon) on its own -- the normal family leaves no pick
undecided, greedy picks are distinct and their gains never increase --, the CLI's new flags, the ctypes table against
include/siggan_diverse.h, the workspace size and every refusal of siggan_select_diverse (argument checks in front of any HIP
call, so they run without a GPU), and diversity_summary's definitions on plain numbers."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from common import ROOT

import diversecommon as D
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib

DIMS, SIZES, PICKS = (1, 3, 4, 5, 40, 128), (1, 2, 63, 64, 65, 257, 1031), 40


def test_normal_family_leaves_no_pick_undecided():
    """The GPU tests compare order[] exactly on this family; that is sound only if no pick is decided by less than 2 B.  The
    cap on cases left out is zero.  Measured when the test was written: the smallest gap is 4.3e8 * B."""
    smallest = math.inf
    for dim in DIMS:
        for n in SIZES:
            order, gain2, count, _, gap, undecided = D.select(D.normal(dim, n), min(PICKS, n))
            assert count == min(PICKS, n)
            assert not undecided.any(), (dim, n, np.flatnonzero(undecided))
            ok = np.isfinite(gap) & (gain2 > 0)
            if ok.any():
                smallest = min(smallest, float((gap[ok] / D.bound(gain2[ok], dim)).min()))
    print(f"smallest gap: {smallest:.3e} * B")
    assert smallest > 2.0


@pytest.mark.parametrize("family", ["normal", "lattice"])
def test_greedy_properties_of_the_yardstick(family):
    for dim in (1, 5, 40):
        for n in (2, 65, 257):
            x = getattr(D, family)(dim, n)
            order, gain2, count, min_d2, _, _ = D.select(x, n)
            assert count == n and sorted(order.tolist()) == list(range(n))          # distinct, and n_select = n empties the set
            finite = gain2[np.isfinite(gain2)]
            assert np.isinf(gain2[0]) and finite.size == n - 1
            assert np.all(finite[1:] <= finite[:-1])                                # after the first finite gain: never larger
            assert np.all(min_d2 == 0.0)


def test_yardstick_stops_masks_and_forces():
    x = np.repeat(D.lattice(5, 20), 3, axis=0)                                       # every row three times
    distinct = len({r.tobytes() for r in x})
    order, gain2, count, _, _, _ = D.select(x, len(x), min_gain2=1e-12)
    assert count == distinct and np.all(order[count:] == -1) and np.all(gain2[count:] == 0.0)
    order, gain2, count, _, _, _ = D.select(x, len(x))
    assert count == len(x) and np.all(gain2[distinct:] == 0.0)                       # duplicates are picked, gain exactly 0
    mask = np.zeros(len(x), np.uint8)
    assert D.select(x, 4, eligible=mask)[2] == 0
    order, _, count, _, _, _ = D.select(x, 4, eligible=mask, first=7)               # the forced row is taken as given
    assert count == 1 and order[0] == 7
    order, gain2, count, _, _, _ = D.select(x, 4, anchor_d2=np.full(len(x), 0.5), min_gain2=1.0)
    assert count == 0                                                                # pick 0 obeys min_gain2


def test_library_exports_the_diverse_header():
    with open(os.path.join(ROOT, "include", "siggan_diverse.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\b(?:int|size_t)\s+(siggan_\w+)\s*\(", header))
    assert declared == set(_lib.DIVERSE_EXPORTS) == {"siggan_select_diverse", "siggan_select_diverse_workspace"}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in siggan_diverse.h but not exported"
    assert lib.siggan_abi_version() == 4                                             # symbols only added
    assert int(re.search(r"#define SIGGAN_DIVERSE_MAX_N\s+(\d+)", header).group(1)) == _lib.DIVERSE_MAX_N == _lib.SELECT_MAX
    assert int(re.search(r"#define SIGGAN_DIVERSE_MAX_DIM\s+(\d+)", header).group(1)) == _lib.DIVERSE_MAX_DIM == _lib.KNN_MAX_DIM
    assert int(re.search(r"#define SIGGAN_DIVERSE_ROW_TILE\s+(\d+)", header).group(1)) == _lib.DIVERSE_ROW_TILE


def test_core_export_list_is_unchanged():
    with open(os.path.join(ROOT, "include", "siggan.h")) as f:
        core = f.read()
    assert not set(_lib.DIVERSE_EXPORTS) & set(_lib.EXPORTS)
    assert all(re.search(rf"\b{name}\s*\(", core) for name in _lib.EXPORTS if name.startswith("siggan_"))
    assert "siggan_select_diverse" not in core
    assert len(_lib.EXPORTS) == 64 and _lib.EXPORTS[0] == "siggan_abi_version" and _lib.EXPORTS[-1] == "mlpgan_op_gemm"


def test_workspace_size():
    lib = _lib.load()
    assert lib.siggan_select_diverse_workspace(0) == 0 and lib.siggan_select_diverse_workspace(-1) == 0
    assert lib.siggan_select_diverse_workspace(_lib.DIVERSE_MAX_N + 1) == 0
    sizes = [lib.siggan_select_diverse_workspace(n) for n in (1, 32, 33, 1031, _lib.DIVERSE_MAX_N)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[0] >= 8 + 1 and sizes[-1] >= 9 * _lib.DIVERSE_MAX_N                # m and the taken flags at the least


def test_every_refusal_comes_before_any_device_call():
    """Host memory stands in for every pointer: a refused call dereferences none and launches nothing."""
    lib = _lib.load()
    n, dim = 8, 4
    buf = (C.c_double * 4096)()
    ptr = C.cast(buf, C.c_void_p)
    size = lib.siggan_select_diverse_workspace(n)

    def call(x=ptr, n=n, dim=dim, first=-1, n_select=3, min_gain2=0.0, order=ptr, gain2=ptr, count=ptr, ws=ptr, ws_bytes=size):
        return lib.siggan_select_diverse(0, x, n, dim, None, None, first, n_select, min_gain2, order, gain2, count, None, ws, ws_bytes, None)

    bad = [dict(n=0), dict(n=-3), dict(n=_lib.DIVERSE_MAX_N + 1, ws_bytes=1 << 30), dict(dim=0), dict(dim=_lib.DIVERSE_MAX_DIM + 1),
           dict(n_select=0), dict(n_select=n + 1), dict(first=-2), dict(first=n), dict(min_gain2=-1e-300), dict(min_gain2=float("nan")),
           dict(x=None), dict(order=None), dict(gain2=None), dict(count=None), dict(ws=None), dict(ws_bytes=size - 1), dict(ws_bytes=0),
           dict(ws=C.c_void_p(ptr.value + 4))]                                        # not 8-byte aligned
    for kw in bad:
        assert call(**kw) == _lib.E_ARG, kw
        assert lib.siggan_last_error(), kw
    assert call(x=None) == _lib.E_ARG and b"null" in lib.siggan_last_error()
    assert call(ws_bytes=size - 1) == _lib.E_ARG and b"workspace" in lib.siggan_last_error()


def test_wrapper_refuses_without_a_device():
    import torch
    from signature_gan_amd.utils.diverse import eligibility, select_diverse
    with pytest.raises(ValueError, match="ROCm device"):
        select_diverse(torch.zeros(9, 8), 3)
    with pytest.raises(ValueError, match="ROCm device"):
        eligibility(torch.zeros(9), 0.5)
    with pytest.raises(ValueError, match="ROCm device"):
        eligibility([0.5, 0.25], 0.5)


def parse(*flags):
    from signature_gan_amd.generate_signatures import parse_args
    return parse_args(["--checkpoint", "ck.pt", *flags])


def refused(capsys, *flags):
    with pytest.raises(SystemExit) as e:
        parse(*flags)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_parse_args_accepts_and_refuses(capsys):
    from signature_gan_amd.generate_signatures import DIVERSE_DEFAULTS, diverse_opt
    base = ("--filter_by_realism", "--diverse", "--verifier_checkpoint", "v.pth")
    plain = parse("--filter_by_realism")
    assert not any(k in vars(plain) for k in DIVERSE_DEFAULTS) and diverse_opt(plain, "diverse") is False
    assert (diverse_opt(plain, "diverse_keep_ratio"), diverse_opt(plain, "diverse_min_separation")) == (0.5, 0.0)
    a = parse(*base)
    assert a.diverse is True and diverse_opt(a, "diverse_keep_ratio") == 0.5 and "diverse_keep_ratio" not in vars(a)
    b = parse(*base, "--diverse_keep_ratio", "0.25", "--diverse_real_dir", "r", "--diverse_memorisation_ratio", "0.5",
              "--diverse_existing_dir", "e", "--diverse_min_separation", "0.1", "--threshold", "127", "--transparent", "--despeckle",
              "--oversampling_ratio", "4", "--noise_scale", "0.9")
    assert (b.diverse_keep_ratio, b.diverse_real_dir, b.diverse_memorisation_ratio, b.diverse_existing_dir, b.diverse_min_separation) == (
        0.25, "r", 0.5, "e", 0.1)
    assert "needs --filter_by_realism" in refused(capsys, "--diverse", "--verifier_checkpoint", "v.pth")
    assert "needs --verifier_checkpoint" in refused(capsys, "--filter_by_realism", "--diverse")
    # the error a verifier checkpoint without --project gave before stays for every command line without --diverse
    assert "need --project" in refused(capsys, "--verifier_checkpoint", "v.pth")
    assert "need --project" in refused(capsys, "--filter_by_realism", "--verifier_checkpoint", "v.pth")
    for flag in (("--diverse_keep_ratio", "0.3"), ("--diverse_real_dir", "r"), ("--diverse_memorisation_ratio", "1"),
                 ("--diverse_existing_dir", "e"), ("--diverse_min_separation", "0.2")):
        assert "need --diverse" in refused(capsys, "--filter_by_realism", *flag)
    assert "need each other" in refused(capsys, *base, "--diverse_real_dir", "r")
    assert "need each other" in refused(capsys, *base, "--diverse_memorisation_ratio", "0.5")
    for other in (("--refine_by_realism",), ("--adapt", "dir"), ("--project", "p"), ("--morph",), ("--pen_width", "3")):
        assert refused(capsys, *base, *other)
    assert refused(capsys, *base, "--diverse_keep_ratio", "0")
    assert refused(capsys, *base, "--diverse_keep_ratio", "1.5")
    assert refused(capsys, *base, "--diverse_min_separation", "-1")


def test_summary_definitions_on_plain_numbers():
    from signature_gan_amd.utils.diverse import diversity_summary
    s = diversity_summary(pool=10, eligible=5, requested=4, order=[3, 7, 1, -1], gain2=[np.inf, 9.0, 4.0, 0.0], count=3,
                          realism=[0.5, 0.25, 0.75], nearest_real_d2=[1.0, 4.0, 16.0], coverage_d2=2.25,
                          selection_nn_d2=[4.0, 4.0, 9.0], top_realism=[0.75, 0.5, 0.5, 0.25], top_nn_d2=[1.0, 1.0, 0.25, 0.25])
    assert (s["pool"], s["eligible"], s["requested"], s["selected"], s["stopped_by"]) == (10, 5, 4, 3, "separation")
    assert s["picks"] == [{"pool_index": 3, "realism": 0.5, "gain": None, "nearest_real": 1.0},
                          {"pool_index": 7, "realism": 0.25, "gain": 3.0, "nearest_real": 2.0},
                          {"pool_index": 1, "realism": 0.75, "gain": 2.0, "nearest_real": 4.0}]
    assert s["coverage_radius"] == 1.5
    assert s["diverse"] == {"min_nn_distance": 2.0, "mean_nn_distance": 7.0 / 3.0, "mean_realism": 0.5}
    assert s["top_n"] == {"min_nn_distance": 0.5, "mean_nn_distance": 0.75, "mean_realism": 0.5}
    kw = dict(order=[2, 0], gain2=[np.inf, 1.0], realism=[0.5, 0.5])
    assert diversity_summary(6, 2, 2, count=2, **kw)["stopped_by"] == "count"
    assert diversity_summary(6, 2, 4, count=2, **kw)["stopped_by"] == "exhausted"
    empty = diversity_summary(6, 0, 4, [-1] * 4, [0.0] * 4, 0, [])
    assert empty["picks"] == [] and empty["stopped_by"] == "exhausted" and empty["coverage_radius"] is None
    assert empty["diverse"] == {"min_nn_distance": None, "mean_nn_distance": None, "mean_realism": None}
    with pytest.raises(ValueError):
        diversity_summary(6, 2, 2, [2, -1], [1.0, 0.0], 2, [0.5, 0.5])
