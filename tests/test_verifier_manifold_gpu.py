"""Precision / recall, density / coverage and nearest-real distances over the Siamese verifier's embeddings on the MI355X:
utils.metrics.calculate_verifier_manifold_metrics and the evaluation CLI's --verifier_neighbors.

Weights: verifier_inputs.gen_state(128), randomly initialised.  Images: 20 "real" and 24 "generated" stroke-like uint8
images (gen_x2_bytes; the generated ones from another seed, with darker ink), k = 3, embedded in chunks of 7.

Yardstick: the numpy twin (utils.neighbors.manifold_from_neighbors) fed with fp64 distances, formed directly as
sum (a - b)^2, of the embeddings the device returned.  Those embeddings come from the GPU, so the margins of the decisions
cannot be fixed in advance by a seed: a comparison the yardstick decides by less than 2 B (B as in test_neighbors_gpu.py)
may be left out here, at most 1 % of them, and the test fails above that.  The exactness claim rests on
test_neighbors_gpu.py, not on this file."""
import glob
import json

import numpy as np
import pytest
import torch

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd.utils.metrics import calculate_verifier_manifold_metrics, verifier_embeddings
from signature_gan_amd.utils.neighbors import manifold_from_neighbors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -52
E, K, N_REAL, N_FAKE, CHUNK = 128, 3, 20, 24, 7
NEW_KEYS = {"verifier_precision", "verifier_recall", "verifier_density", "verifier_coverage", "verifier_nearest_real",
            "verifier_neighbors_k"}

_CASE = {}


def case():
    """Computed once and left unchanged: the model, both image sets on the device, their embeddings on the host (fp64)."""
    if not _CASE:
        from signature_gan_amd import signature_verifier_eval as SV
        model = SV.SiameseNetwork(E, max_images=64)
        model.load_state_dict(VC.torch_state(E), strict=True)
        model = model.to(DEV).eval()
        real = torch.from_numpy(VI.gen_x2_bytes(N_REAL)).to(DEV)
        other = VI.gen_x2_bytes(N_FAKE, seed=VI.SEED["x2"] + 1)
        fake = torch.from_numpy(np.where(other < 255, other // 2, 255).astype(np.uint8)).to(DEV)
        emb = [verifier_embeddings(x, model, CHUNK).cpu().double().numpy() for x in (real, fake)]
        _CASE.update(model=model, real=real, fake=fake, emb=emb)
    return _CASE


def pairwise(a, b):
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    return d2, (a.shape[1] + 4) * U * (na[:, None] + nb[None, :]) ** 2


def host_metrics(real, fake, k):
    """(the twin's dictionary from fp64 distances, comparisons made, comparisons with a margin under 2 B)."""
    rr, b_rr = pairwise(real, real)
    ff, b_ff = pairwise(fake, fake)
    fr, b_fr = pairwise(fake, real)
    rr_x, ff_x = rr.copy(), ff.copy()
    np.fill_diagonal(rr_x, np.inf)
    np.fill_diagonal(ff_x, np.inf)
    made = close = 0

    def kth(d2x, bound):
        nonlocal made, close
        order = np.argsort(d2x, axis=1, kind="stable")
        rows = np.arange(d2x.shape[0])[:, None]
        s, b = d2x[rows, order[:, :k + 1]], bound[rows, order[:, :k + 1]]
        gaps = (s[:, 1:] - s[:, :-1]) <= 2 * np.maximum(b[:, 1:], b[:, :-1])
        made, close = made + gaps.size, close + int(gaps.sum())
        return s[:, k - 1], s[:, 0]

    radius2_real, real_loo = kth(rr_x, b_rr)
    radius2_fake, _ = kth(ff_x, b_ff)
    for d2, bound, radius2 in ((fr, b_fr, radius2_real[None, :]), (fr.T, b_fr.T, radius2_fake[None, :])):
        tight = np.abs(d2 - radius2) <= 2 * bound
        made, close = made + tight.size, close + int(tight.sum())
    for d2, bound, radius2 in ((fr.T, b_fr.T, radius2_real), (fr, b_fr, None)):          # the two 1-nearest-neighbour queries
        s, b = np.sort(d2, axis=1)[:, :2], np.sort(bound, axis=1)[:, -1:]
        tight = (s[:, 1] - s[:, 0]) <= 2 * b[:, 0]
        if radius2 is not None:                                                         # coverage's comparison
            tight = tight | (np.abs(s[:, 0] - radius2) <= 2 * b[:, 0])
        made, close = made + tight.size, close + int(tight.sum())
    want = manifold_from_neighbors(k, radius2_real, radius2_fake, (fr <= radius2_real[None, :]).sum(axis=1),
                                   (fr.T <= radius2_fake[None, :]).sum(axis=1), fr.min(axis=0), fr.min(axis=1),
                                   fr.argmin(axis=1), real_loo)
    return want, made, close, float(max(b_rr.max(), b_ff.max(), b_fr.max()))


def test_metrics_of_two_image_sets():
    c = case()
    got = calculate_verifier_manifold_metrics(c["real"], c["fake"], c["model"], k=K, max_batch=CHUNK)
    want, made, close, b_max = host_metrics(c["emb"][0], c["emb"][1], K)
    print(f"comparisons {made}, with a margin under 2 B {close}; B <= {b_max:.3e}")
    for key in ("precision", "recall", "density", "coverage"):
        print(f"{key}: {got[key]!r} host {want[key]!r}")
    print(f"nearest_real: {got['nearest_real']} host {want['nearest_real']}")
    assert close <= 0.01 * made, f"{close} of {made} comparisons have a margin under 2 B: more than 1 % would be left out"
    assert (got["k"], got["n_real"], got["n_generated"], got["embedding_dim"]) == (K, N_REAL, N_FAKE, E)
    for key in ("radius2_real", "radius2_fake"):
        assert got[key].dtype == np.float64 and got[key].shape == want[key].shape
        assert (np.abs(got[key] - want[key]) <= 2 * b_max).all(), key
    # every decision with a margin agrees; each one without may move a mean by one sample
    for key, n in (("precision", N_FAKE), ("recall", N_REAL), ("coverage", N_REAL)):
        assert abs(got[key] - want[key]) <= close / n + 1e-15, key
    assert abs(got["density"] - want["density"]) <= close / (K * N_FAKE) + 1e-15
    g, w = got["nearest_real"], want["nearest_real"]
    root_tol = b_max / min(w["min"], w["real_loo_median"])                # |sqrt a - sqrt b| <= |a - b| / sqrt b
    for key in ("mean", "median", "min", "real_loo_median"):
        assert abs(g[key] - w[key]) <= root_tol, key
    assert g["ratio_median"] == g["median"] / g["real_loo_median"] and 0 < g["min"] <= g["median"]
    assert len(g["closest"]) == 5
    if close == 0:
        assert [(a, b) for a, b, _ in g["closest"]] == [(a, b) for a, b, _ in w["closest"]]
    assert all(abs(d - dw) <= root_tol for (_, _, d), (_, _, dw) in zip(g["closest"], w["closest"]))
    # two different sets of random images through random weights: neither collapsed onto the other
    assert 0.0 <= got["precision"] <= 1.0 and 0.0 <= got["recall"] <= 1.0 and got["density"] >= 0.0
    # the encoder alone gives the same embeddings, hence the same figures
    enc = calculate_verifier_manifold_metrics(c["real"], c["fake"], c["model"].encoder.eval(), k=K, max_batch=CHUNK)
    assert enc["nearest_real"] == got["nearest_real"] and all(enc[key] == got[key] for key in ("precision", "recall", "density", "coverage"))


def test_a_set_against_itself():
    c = case()
    got = calculate_verifier_manifold_metrics(c["real"], c["real"], c["model"], k=K, max_batch=CHUNK)
    assert got["precision"] == got["recall"] == got["coverage"] == 1.0 and got["density"] >= 1.0 / K
    nr = got["nearest_real"]
    assert nr["mean"] == nr["median"] == nr["min"] == 0.0 and nr["ratio_median"] == 0.0 and nr["real_loo_median"] > 0
    assert [(a, b, d) for a, b, d in nr["closest"]] == [(i, i, 0.0) for i in range(5)]
    assert np.array_equal(got["radius2_real"], got["radius2_fake"])
    for n_real, n_fake in ((K, N_FAKE), (N_REAL, K)):
        with pytest.raises(ValueError, match="more than k"):
            calculate_verifier_manifold_metrics(c["real"][:n_real], c["fake"][:n_fake], c["model"], k=K)


def test_evaluate_cli_with_neighbors(tmp_path, capsys):
    """A tiny Generator checkpoint, a verifier checkpoint, 40 samples at batch 16 and 12 PNGs: with --verifier_neighbors 3
    the report holds the new keys; the same command without it writes exactly the keys it wrote before."""
    from PIL import Image
    from common import I, O, SEED
    from signature_gan_amd import evaluate_vanilla_gan_signatures as cli
    from signature_gan_amd.generator_vanilla_gan import Generator
    size, latent = 64, 100
    g = Generator(latent_dim=latent, output_size=size)
    g.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in I.gen_state(O.g_state_specs(latent, size), SEED["state_g"]).items()})
    ck, vck = tmp_path / "ck.pt", tmp_path / "verifier.pth"
    torch.save({"epoch": 2, "generator_state_dict": {k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
                "config": {"latent_dim": latent, "image_size": size, "current_epoch": 2}}, ck)
    torch.save({"model_state_dict": VC.torch_state(128), "embedding_dim": 128, "val_accuracy": 0.9, "epoch": 1}, vck)
    real_dir = tmp_path / "real"
    real_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(12):
        a = np.where(rng.uniform(size=(40, 52)) < 0.1, rng.integers(0, 128, (40, 52)), 255).astype(np.uint8)
        Image.fromarray(a, "L").save(real_dir / f"r{i:02d}.png")

    def run(name, *extra):
        out = tmp_path / name
        rc = cli.main(["--checkpoint", str(ck), "--n_samples", "40", "--batch_size", "16", "--n_grids", "0", "--seed", "3",
                       "--output_dir", str(out), *extra])
        text = capsys.readouterr().out
        reports = glob.glob(str(out / "evaluation_report_*.json"))
        assert rc == 0 and len(reports) == 1, text
        with open(reports[0]) as f:
            return json.load(f), text

    before, text_before = run("a", "--real_dir", str(real_dir), "--verifier_checkpoint", str(vck))
    assert not NEW_KEYS & set(before["metrics"]) and "Precision" not in text_before and "Recall" not in text_before
    with_flag, text = run("b", "--real_dir", str(real_dir), "--verifier_checkpoint", str(vck), "--verifier_neighbors", "3")
    m = with_flag["metrics"]
    assert set(m) == set(before["metrics"]) | NEW_KEYS and "verifier_neighbors_error" not in m
    assert set(with_flag["summary"]) == set(before["summary"]) | {"verifier_precision", "verifier_recall"}
    assert m["verifier_neighbors_k"] == 3
    for key in ("verifier_precision", "verifier_recall", "verifier_coverage"):
        assert 0.0 <= m[key] <= 1.0, key
    assert m["verifier_density"] >= 0.0
    nr = m["verifier_nearest_real"]
    assert set(nr) == {"mean", "median", "min", "real_loo_median", "ratio_median", "closest"}
    assert 0 < nr["min"] <= nr["median"] and nr["real_loo_median"] > 0 and len(nr["closest"]) == 5
    assert all(0 <= a < 40 and 0 <= b < 12 and d >= nr["min"] for a, b, d in nr["closest"]) and nr["closest"][0][2] == nr["min"]
    assert with_flag["summary"]["verifier_precision"] == m["verifier_precision"]
    assert with_flag["summary"]["verifier_recall"] == m["verifier_recall"]
    assert f"Verifier Precision: {m['verifier_precision']:.4f} (generated samples inside the real manifold, k = 3)" in text
    assert f"Verifier Recall: {m['verifier_recall']:.4f} (real samples inside the generated manifold, k = 3)" in text
    # the flag changes nothing else: the same seed's samples, the same figures
    for key in set(before["metrics"]) - {"metrics_computed_at"}:
        assert before["metrics"][key] == m[key], key

    # a run without either flag has the keys of a run that knows neither
    plain, text_plain = run("c", "--real_dir", str(real_dir))
    assert not [k for k in plain["metrics"] if k.startswith("verifier")] and "erifier" not in text_plain

    no_real, text = run("d", "--verifier_checkpoint", str(vck), "--verifier_neighbors", "3")
    assert no_real["metrics"]["verifier_precision"] is None and no_real["metrics"]["verifier_nearest_real"] is None
    assert no_real["metrics"]["verifier_neighbors_error"] == "no real images provided"
    assert no_real["summary"]["verifier_recall"] is None
    assert "Verifier Precision: Not computed - no real images provided" in text

    no_verifier, _ = run("e", "--real_dir", str(real_dir), "--verifier_neighbors", "3")
    assert "--verifier_checkpoint" in no_verifier["metrics"]["verifier_neighbors_error"]
    assert no_verifier["metrics"]["verifier_precision"] is None

    too_many, _ = run("f", "--real_dir", str(real_dir), "--verifier_checkpoint", str(vck), "--verifier_neighbors", "12")
    assert "more than k" in too_many["metrics"]["verifier_neighbors_error"] and too_many["metrics"]["verifier_recall"] is None
