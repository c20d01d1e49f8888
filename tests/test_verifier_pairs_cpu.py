"""All-pairs scoring, host side: metrics_from_counts against compute_verification_metrics, its brackets under a coarse grid,
the default threshold grid, the host refusals, and the new header's exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF32 = np.float32(np.inf)


def counts(scores, labels, grid):
    """The two (T + 1) histograms siggan_verifier_pairs would return for these fp32 scores."""
    b = np.searchsorted(grid, scores, side="right")
    n = grid.size + 1
    return np.bincount(b[labels == 1], minlength=n), np.bincount(b[labels == 0], minlength=n)


def scores_and_labels(rng, n_genuine, n_impostor, ties):
    s = np.concatenate([rng.beta(5, 2, n_genuine), rng.beta(2, 5, n_impostor)]).astype(np.float32)
    if ties:                                                # a coarse lattice: many equal scores across the classes
        s = (np.round(s * 64) / 64).astype(np.float32)
    y = np.r_[np.ones(n_genuine, np.int64), np.zeros(n_impostor, np.int64)]
    return s, y


def reference(s, y, threshold):
    s64 = s.astype(np.float64)
    return SV.compute_verification_metrics(y, s64, (s64 >= threshold).astype(int), threshold)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("threshold", [0.5, 0.3, 0.7])
def test_metrics_from_counts_equal_the_metrics_from_scores_on_a_full_grid(ties, threshold):
    rng = np.random.default_rng(11 + int(ties))
    s, y = scores_and_labels(rng, 300, 900, ties)
    # every distinct score and the next float32 above it: each occupied bin provably holds one value
    d = np.unique(s)
    grid = np.unique(np.concatenate([d, np.nextafter(d, INF32), [SV.threshold_as_float32(threshold)]]).astype(np.float32))
    g, im = counts(s, y, grid)
    got, want = SV.metrics_from_counts(grid, g, im, threshold), reference(s, y, threshold)
    assert set(got) == set(want) | {"roc_auc_bounds", "eer_bounds"}
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12, (k, got[k], v)
    for k in ("true_positives", "true_negatives", "false_positives", "false_negatives", "total_genuine", "total_forgeries"):
        assert got[k] == want[k] and isinstance(got[k], int)
    assert got["roc_auc_bounds"] == [got["roc_auc"], got["roc_auc"]]
    assert got["eer_bounds"] == [got["eer"], got["eer"]]
    # the distinct scores alone: the same values (only the brackets need the proof that a bin holds one value)
    grid2 = np.unique(np.concatenate([d, [SV.threshold_as_float32(threshold)]]).astype(np.float32))
    got2 = SV.metrics_from_counts(grid2, *counts(s, y, grid2), threshold)
    for k, v in want.items():
        assert abs(got2[k] - v) <= 1e-12, (k, got2[k], v)


def test_coarse_grid_brackets_hold_the_true_auc_and_eer():
    """200 seeded trials at a class imbalance of 1:50, grids of 5 .. 200 values, with and without tied scores."""
    rng = np.random.default_rng(2024)
    widths = []
    for trial in range(200):
        n_gen = int(rng.integers(8, 40))
        s, y = scores_and_labels(rng, n_gen, 50 * n_gen, ties=bool(trial & 1))
        T = int(rng.integers(5, 200))
        grid = np.unique(np.concatenate([rng.random(T), [0.5]]).astype(np.float32))
        m = SV.metrics_from_counts(grid, *counts(s, y, grid), 0.5)
        want = reference(s, y, 0.5)
        lo, hi = m["roc_auc_bounds"]
        assert lo - 1e-12 <= want["roc_auc"] <= hi + 1e-12, (trial, lo, want["roc_auc"], hi)
        assert lo - 1e-12 <= m["roc_auc"] <= hi + 1e-12
        lo, hi = m["eer_bounds"]
        assert lo - 1e-12 <= want["eer"] <= hi + 1e-12, (trial, lo, want["eer"], hi)
        widths.append(hi - lo)
        for k in ("accuracy", "far", "frr", "true_positives", "false_positives", "true_negatives", "false_negatives"):
            assert m[k] == want[k], (trial, k)                       # exact at the threshold whatever the grid
    assert np.median(widths) < 0.5                                    # a bracket, not [0, 1]


def test_metrics_from_counts_refusals():
    grid = np.array([0.25, 0.5, 0.75], np.float32)
    g, im = np.array([1, 2, 3, 4]), np.array([4, 3, 2, 1])
    SV.metrics_from_counts(grid, g, im, 0.5)
    with pytest.raises(ValueError):
        SV.metrics_from_counts(grid, g, im, 0.4)                      # not a grid value
    with pytest.raises(ValueError):
        SV.metrics_from_counts(grid, g[:3], im, 0.5)
    with pytest.raises(ValueError):
        SV.metrics_from_counts(grid[::-1], g, im, 0.5)


@pytest.mark.parametrize("threshold", [0.5, 0.3, 0.123456789, 0.0, 1.0])
def test_default_threshold_grid(threshold):
    grid = SV.default_threshold_grid(threshold)
    assert grid.dtype == np.float32 and grid.ndim == 1
    assert grid.size <= _lib.PAIR_MAX_THRESHOLDS == 4096
    assert np.all(np.diff(grid) > 0)                                  # sorted and unique
    t32 = SV.threshold_as_float32(threshold)
    assert t32 in grid and float(t32) >= threshold and float(np.nextafter(t32, -INF32)) < threshold
    assert np.all(np.isin((np.arange(1025) / 1024).astype(np.float32), grid))
    assert grid[0] == 0.0 and grid[-1] == 1.0
    assert np.sum(grid < 1e-4) > 100 and np.sum(grid > 1 - 1e-4) > 100       # resolution where saturated scores live


def test_host_refusals_need_no_device():
    e = torch.zeros(4, 128)
    ids = torch.zeros(4, dtype=torch.int32)
    ok = dict(e_q=e, ids_q=ids, e_r=e, ids_r=ids, same_set=True, want_matrix=False, thresholds=[0.5], want_best=False, embedding_dim=128)
    assert SV.check_pairs_args(**ok)[:2] == (4, 4)
    bad = [dict(thresholds=None),                                     # no output requested
           dict(thresholds=[]), dict(thresholds=np.zeros(4097)), dict(thresholds=[0.5, 0.25]), dict(thresholds=[float("nan")]),
           dict(e_r=torch.zeros(5, 128), ids_r=torch.zeros(5, dtype=torch.int32)),         # same_set with nq != nr
           dict(e_q=torch.zeros(4, 64)), dict(e_q=e.double()), dict(e_q=torch.zeros(0, 128), ids_q=None),
           dict(ids_q=ids.long()), dict(ids_q=torch.zeros(3, dtype=torch.int32)),
           dict(e_q=torch.zeros(4, 1025), e_r=torch.zeros(4, 1025), embedding_dim=1025)]
    for change in bad:
        with pytest.raises(ValueError):
            SV.check_pairs_args(**{**ok, **change})
    m = SV.SiameseNetwork(128)
    with pytest.raises(ValueError):
        m.pairs(e, None, e, None)                                     # refused before the device is looked at
    with pytest.raises(RuntimeError):
        m.eval().score_matrix(e, e)                                   # CPU tensors: no CPU path


def test_library_exports_the_pairs_header():
    with open(os.path.join(ROOT, "include", "siggan_verifier_pairs.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\bint\s+(siggan_verifier_\w+)\s*\(", text))
    assert declared == {"siggan_verifier_pairs_enable", "siggan_verifier_pairs"}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in siggan_verifier_pairs.h but not exported"
    assert declared == set(_lib.VERIFIER_PAIRS_EXPORTS)
    bound = _lib.load()
    for name in declared:
        assert getattr(bound, name).argtypes is not None
    assert int(re.search(r"#define\s+SIGGAN_PAIR_MAX_DIM\s+(\d+)", text).group(1)) == _lib.PAIR_MAX_DIM
    assert int(re.search(r"#define\s+SIGGAN_PAIR_MAX_THRESHOLDS\s+(\d+)", text).group(1)) == _lib.PAIR_MAX_THRESHOLDS
    # the structure's fields, in the header's order
    body = re.search(r"typedef struct siggan_pair_outputs \{(.*?)\} siggan_pair_outputs;", text, re.S).group(1)
    fields = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert fields == [n for n, _ in _lib.PairOutputs._fields_]
    lib.siggan_abi_version.restype = C.c_int
    assert lib.siggan_abi_version() == 4
