"""CPU-only checks of the nearest-neighbour metrics: the numpy twin of the definitions (utils.neighbors.
manifold_from_neighbors) on hand-made sets whose answers are known, the size rule, the ctypes table against
include/siggan_neighbors.h, the library's refusals (which touch no device) and the CLI flag."""
import os
import re

import numpy as np
import pytest

from common import ROOT

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils.neighbors import manifold_from_neighbors, manifold_metrics


def neighbor_data(real, fake, k):
    """What the six device launches hand the twin, restated with a dense fp64 distance matrix."""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)

    def d2(a, b):
        return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)

    rr, ff, fr = d2(real, real), d2(fake, fake), d2(fake, real)
    np.fill_diagonal(rr, np.inf)
    np.fill_diagonal(ff, np.inf)
    radius2_real, radius2_fake = np.sort(rr, axis=1)[:, k - 1], np.sort(ff, axis=1)[:, k - 1]
    return dict(k=k, radius2_real=radius2_real, radius2_fake=radius2_fake,
                fake_in_real=(fr <= radius2_real[None, :]).sum(axis=1), real_in_fake=(fr.T <= radius2_fake[None, :]).sum(axis=1),
                real_to_fake_d2=fr.min(axis=0), fake_to_real_d2=fr.min(axis=1), fake_to_real_index=fr.argmin(axis=1),
                real_loo_d2=rr.min(axis=1))


def grid(n, origin):
    """n x n points with spacing 1 from ``origin``: every point has neighbours at distance 1."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n)), axis=-1).reshape(-1, 2).astype(np.float64)
    return g + np.asarray(origin, np.float64)


def test_identical_sets():
    x = grid(4, (0, 0))
    m = manifold_from_neighbors(**neighbor_data(x, x, 3))
    assert m["precision"] == m["recall"] == m["coverage"] == 1.0
    assert m["density"] >= 1.0                               # every sample lies in its own ball and in its neighbours'
    nr = m["nearest_real"]
    assert nr["mean"] == nr["median"] == nr["min"] == 0.0 and nr["real_loo_median"] == 1.0 and nr["ratio_median"] == 0.0
    assert nr["closest"] == [(i, i, 0.0) for i in range(5)]   # equal distances: by generated index
    assert m["k"] == 3 and m["n_real"] == m["n_generated"] == 16
    assert np.array_equal(m["radius2_real"], m["radius2_fake"])


def test_far_apart_sets():
    m = manifold_from_neighbors(**neighbor_data(grid(3, (0, 0)), grid(3, (1000, 1000)), 2))
    assert (m["precision"], m["recall"], m["coverage"], m["density"]) == (0.0, 0.0, 0.0, 0.0)
    assert m["nearest_real"]["min"] == pytest.approx(np.hypot(998, 998))
    assert m["nearest_real"]["ratio_median"] > 100


def test_generated_set_on_one_of_two_real_clusters():
    a, b = grid(3, (0, 0)), grid(3, (1000, 0))
    real = np.concatenate([a, b])
    fake = a + 0.01                                          # sits on cluster a only
    m = manifold_from_neighbors(**neighbor_data(real, fake, 2))
    assert m["precision"] == 1.0 and m["recall"] == 0.5 and m["coverage"] == 0.5
    assert m["density"] == pytest.approx(neighbor_data(real, fake, 2)["fake_in_real"].sum() / (2 * 9))
    nr = m["nearest_real"]
    assert nr["median"] == pytest.approx(0.01 * np.sqrt(2)) and nr["real_loo_median"] == 1.0
    assert nr["ratio_median"] == pytest.approx(0.01 * np.sqrt(2))          # far below 1: the memorisation warning
    assert len(nr["closest"]) == 5 and all(g == r and d == pytest.approx(0.01 * np.sqrt(2)) for g, r, d in nr["closest"])


def test_definitions_on_plain_numbers():
    """No geometry at all: counts and distances in, the formulas out."""
    m = manifold_from_neighbors(k=2, radius2_real=[1.0, 4.0, 9.0], radius2_fake=[1.0, 1.0, 1.0, 1.0],
                                fake_in_real=[0, 3, 1, 0], real_in_fake=[2, 0, 0],
                                real_to_fake_d2=[1.0, 4.5, 0.25], fake_to_real_d2=[16.0, 0.25, 4.0, 9.0],
                                fake_to_real_index=[2, 0, 1, 1], real_loo_d2=[4.0, 4.0, 16.0])
    assert m["precision"] == 0.5 and m["recall"] == pytest.approx(1 / 3) and m["density"] == 4 / (2 * 4)
    assert m["coverage"] == pytest.approx(2 / 3)             # 1 <= 1 (a tie counts), 4.5 > 4, 0.25 <= 9
    nr = m["nearest_real"]
    assert (nr["mean"], nr["median"], nr["min"], nr["real_loo_median"], nr["ratio_median"]) == (2.375, 2.5, 0.5, 2.0, 1.25)
    assert nr["closest"] == [(1, 0, 0.5), (2, 1, 2.0), (3, 1, 3.0), (0, 2, 4.0)]
    degenerate = manifold_from_neighbors(k=1, radius2_real=[0.0, 0.0], radius2_fake=[0.0, 0.0], fake_in_real=[1, 1],
                                         real_in_fake=[1, 1], real_to_fake_d2=[0.0, 0.0], fake_to_real_d2=[0.0, 0.0],
                                         fake_to_real_index=[0, 1], real_loo_d2=[0.0, 0.0])
    assert degenerate["nearest_real"]["ratio_median"] is None              # no division by a zero median


def test_too_few_samples_are_refused():
    x = grid(2, (0, 0))                                      # 4 samples
    for k in (4, 5):
        with pytest.raises(ValueError, match="more than k"):
            manifold_from_neighbors(k=k, radius2_real=np.ones(4), radius2_fake=np.ones(9), fake_in_real=np.ones(9, int),
                                    real_in_fake=np.ones(4, int), real_to_fake_d2=np.ones(4), fake_to_real_d2=np.ones(9),
                                    fake_to_real_index=np.zeros(9, int), real_loo_d2=np.ones(4))
    with pytest.raises(ValueError, match="more than k"):
        manifold_from_neighbors(**dict(neighbor_data(grid(3, (0, 0)), x, 3), k=4))
    with pytest.raises(ValueError):
        manifold_from_neighbors(k=0, **{k_: v for k_, v in neighbor_data(x, x, 1).items() if k_ != "k"})
    with pytest.raises(ValueError, match="entries"):
        manifold_from_neighbors(**dict(neighbor_data(x, x, 1), real_loo_d2=np.ones(3)))
    # the device entry point refuses on the sizes before it looks for a device
    import torch
    with pytest.raises(ValueError, match="more than k"):
        manifold_metrics(torch.zeros(3, 8), torch.zeros(9, 8), k=3)
    with pytest.raises(ValueError, match="ROCm device"):
        manifold_metrics(torch.zeros(9, 8), torch.zeros(9, 8), k=3)


def test_library_exports_the_neighbors_header():
    with open(os.path.join(ROOT, "include", "siggan_neighbors.h")) as f:
        header = f.read()
    declared = set(re.findall(r"\bint\s+(siggan_\w+)\s*\(", header))
    assert declared == set(_lib.NEIGHBORS_EXPORTS) == {"siggan_knn", "siggan_ball_count"}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in siggan_neighbors.h but not exported"
    assert lib.siggan_abi_version() == 4                   # symbols only added
    assert int(re.search(r"#define SIGGAN_KNN_MAX_K\s+(\d+)", header).group(1)) == _lib.KNN_MAX_K
    assert int(re.search(r"#define SIGGAN_KNN_MAX_DIM\s+(\d+)", header).group(1)) == _lib.KNN_MAX_DIM
    # refused before anything touches a device
    assert lib.siggan_knn(0, None, 4, None, 4, 8, 1, 0, None, None, None) == _lib.E_ARG and b"null" in lib.siggan_last_error()
    assert lib.siggan_ball_count(0, None, 4, None, 4, 8, None, None, None) == _lib.E_ARG and b"null" in lib.siggan_last_error()


def test_cli_flag_is_opt_in():
    from signature_gan_amd.evaluate_vanilla_gan_signatures import parse_args
    a = parse_args(["--checkpoint", "ck.pt"])
    assert a.verifier_neighbors is None and "verifier_neighbors" not in vars(a)
    b = parse_args(["--checkpoint", "ck.pt", "--verifier_checkpoint", "v.pth", "--real_dir", "r", "--verifier_neighbors", "3"])
    assert b.verifier_neighbors == 3 and vars(b)["verifier_neighbors"] == 3


def test_report_without_the_flag_keeps_its_keys(tmp_path, capsys):
    """save_evaluation_report / print_summary on ready metrics: the precision / recall lines and summary keys appear only
    when the metrics hold them."""
    import json
    from signature_gan_amd.evaluate_vanilla_gan_signatures import print_summary, save_evaluation_report
    base = {"n_samples": 4, "image_shape": [1, 64, 64], "fid_score": None, "lpips_diversity": None,
            "stroke_density": {"mean": 0.25, "std": 0.0, "min": 0.25, "max": 0.25},
            "foreground_ratio": {"mean": 0.25, "std": 0.0, "percentiles": {"25": 0.25, "50": 0.25, "75": 0.25}}}

    def run(metrics, name):
        path = save_evaluation_report(metrics, {}, tmp_path / name, "ck.pt", [])
        print_summary(metrics)
        with open(path) as f:
            return json.load(f)["summary"], capsys.readouterr().out

    plain, text = run(dict(base), "a")
    assert "verifier_precision" not in plain and "verifier_recall" not in plain and "erifier" not in text
    with_keys, text = run(dict(base, verifier_precision=0.75, verifier_recall=0.5, verifier_neighbors_k=3), "b")
    assert set(with_keys) == set(plain) | {"verifier_precision", "verifier_recall"}
    assert (with_keys["verifier_precision"], with_keys["verifier_recall"]) == (0.75, 0.5)
    lines = text.splitlines()
    at = lines.index("Verifier Precision: 0.7500 (generated samples inside the real manifold, k = 3)")
    assert lines.index("--- Quality Metrics ---") < at < lines.index("--- Stroke Analysis ---")
    assert "Verifier Recall: 0.5000 (real samples inside the generated manifold, k = 3)" in lines
    failed, text = run(dict(base, verifier_precision=None, verifier_recall=None, verifier_neighbors_k=3,
                            verifier_neighbors_error="no real images provided"), "c")
    assert failed["verifier_precision"] is None and "Verifier Precision: Not computed - no real images provided" in text
