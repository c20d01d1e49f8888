"""Frechet distance over the Siamese verifier's embeddings on the MI355X: the streaming path (embed_u8 / forward_one ->
FeatureMoments), utils.metrics.calculate_verifier_frechet_distance and the evaluation CLI's --verifier_checkpoint.

Weights: verifier_inputs.gen_state(E), E = 40 and 128.  Images: gen_x2_bytes (uint8, stroke-like; the "real" set) and
gen_x1 (fp32 noise; the "generated" set), 96 per set for E = 40 and 160 for E = 128, so n > E and both covariances have
full rank.

The moments are held to test_moments_gpu's bound against numpy fp64 moments of the SAME device embeddings copied to the
host.  The distance is compared with frechet_distance on np.cov of those embeddings; its tolerance cannot be derived in
advance, because sqrtm amplifies a perturbation of the covariances by their conditioning.  It was measured on the CPU
(``cpu_sensitivity``; this file run as a script with the repository root on PYTHONPATH prints it): embeddings of the
same inputs from verifiercommon.encode, G and s of both sets perturbed by the moments bound with random signs, 8 draws,
the largest change of the distance --

    E = 40,  n = 96:   distance 0.1537, tr(cov_1) + tr(cov_2) = 0.0262, largest change 2.99e-14  (1.1e-12 of the traces)
    E = 128, n = 160:  distance 0.1523, tr(cov_1) + tr(cov_2) = 0.0279, largest change 5.05e-14  (1.8e-12 of the traces)

-- six orders below the 1e-6 of the traces at which the inputs would have had to change (random weights put all
embeddings close together, hence the small traces; the covariances still have full rank).  TOLERANCE is 16 x the
measured change; the factor covers the difference between the CPU restatement's embeddings and the device's."""
import glob
import json
import math

import numpy as np
import pytest
import torch

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd.utils.frechet import FeatureMoments, frechet_distance, stats_from_moments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U2 = 2.0 ** -52
N_IMAGES = {40: 96, 128: 160}
MEASURED_CHANGE = {40: 2.99e-14, 128: 5.05e-14}             # cpu_sensitivity(e), see the module docstring
FACTOR = 16.0
TOLERANCE = {e: FACTOR * v for e, v in MEASURED_CHANGE.items()}


def image_sets(e):
    n = N_IMAGES[e]
    return torch.from_numpy(VI.gen_x2_bytes(n)), torch.from_numpy(VI.gen_x1(n))


def moments_bound(x):
    """(bound on s, bound on G) for fp64 rows x."""
    ax = np.abs(x)
    return x.shape[0] * U2 * ax.sum(axis=0), x.shape[0] * U2 * (ax.T @ ax)


def cpu_sensitivity(e, draws=8):
    """(distance, sum of traces, largest change of the distance) when both sets' moments move by their bound."""
    real, fake = image_sets(e)
    sd = VC.torch_state(e)
    with torch.no_grad():
        sets = [VC.encode(sd, torch.from_numpy(VI.normalize_bytes(real.numpy()))[:, None]).double().numpy(),
                VC.encode(sd, fake).double().numpy()]
    base = [stats_from_moments(x.shape[0], x.sum(axis=0), x.T @ x) for x in sets]
    d0 = frechet_distance(base[0][1], base[0][2], base[1][1], base[1][2])
    rng = np.random.default_rng(e)
    worst = 0.0
    for _ in range(draws):
        moved = []
        for x in sets:
            bs, bg = moments_bound(x)
            sg = np.triu(rng.choice([-1.0, 1.0], bg.shape))
            sg = sg + np.triu(sg, 1).T                                      # the device's G is exactly symmetric
            moved.append(stats_from_moments(x.shape[0], x.sum(axis=0) + rng.choice([-1.0, 1.0], bs.shape) * bs, x.T @ x + sg * bg))
        worst = max(worst, abs(frechet_distance(moved[0][1], moved[0][2], moved[1][1], moved[1][2]) - d0))
    return d0, float(np.trace(base[0][2]) + np.trace(base[1][2])), worst


def make_model(e, max_images):
    from signature_gan_amd import signature_verifier_eval as SV
    m = SV.SiameseNetwork(e, max_images=max_images)
    m.load_state_dict(VC.torch_state(e), strict=True)
    return m.to(DEV).eval()


_CASES = {}


def case(e):
    """Per E, computed once and left unchanged: the model, both image sets on the device, their embeddings on the host
    (fp64) and the host-side statistics of those."""
    if e not in _CASES:
        model = make_model(e, 64)
        real, fake = (t.to(DEV) for t in image_sets(e))
        emb = [model.embed_u8(real).cpu().double().numpy(), model.forward_one(fake).cpu().double().numpy()]
        host = [(x.mean(axis=0), np.cov(x, rowvar=False)) for x in emb]
        _CASES[e] = dict(model=model, real=real, fake=fake, emb=emb, host=host)
    return _CASES[e]


@pytest.mark.parametrize("e", [40, 128])
def test_streaming_moments_of_embeddings(e):
    """Uneven chunks (32, 32, ..., n - 1 - 32 k, 1) through embed_u8 / forward_one into FeatureMoments."""
    c = case(e)
    n = N_IMAGES[e]
    cuts = list(range(0, n - 1, 32)) + [n - 1, n]
    assert cuts[-2] - cuts[-3] == 31 and cuts[-1] - cuts[-2] == 1
    for images, embed, x, what in ((c["real"], c["model"].embed_u8, c["emb"][0], "bytes"),
                                   (c["fake"], c["model"].forward_one, c["emb"][1], "fp32")):
        m = FeatureMoments(e, DEV)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            m.update(embed(images[lo:hi]))
        count, s, g = m.read()
        bs, bg = moments_bound(x)
        e_s, e_g = np.abs(s - x.sum(axis=0)), np.abs(g - x.T @ x)
        print(f"E={e} {what}: worst s error / bound {float((e_s / bs).max()):.3e}, worst G error / bound {float((e_g / bg).max()):.3e}")
        assert count == n and (e_s <= bs).all() and (e_g <= bg).all() and np.array_equal(g, g.T)
        assert abs(np.trace(g) - n) <= 1e-5 * n                              # unit-norm embeddings
        m.close()


@pytest.mark.parametrize("e", [40, 128])
def test_distance_of_the_two_sets(e):
    from signature_gan_amd.utils.metrics import calculate_verifier_frechet_distance
    c = case(e)
    (mu_r, cov_r), (mu_f, cov_f) = c["host"]
    want = frechet_distance(mu_r, cov_r, mu_f, cov_f)
    traces = float(np.trace(cov_r) + np.trace(cov_f))
    got = calculate_verifier_frechet_distance(c["real"], c["fake"], c["model"], max_batch=40)
    print(f"E={e}: distance {got['frechet_distance']!r} host {want!r} difference {abs(got['frechet_distance'] - want):.3e} "
          f"tolerance {TOLERANCE[e]:.3e} traces {traces:.4f}")
    assert set(got) == {"frechet_distance", "spread_real", "spread_generated", "n_real", "n_generated", "embedding_dim"}
    assert (got["n_real"], got["n_generated"], got["embedding_dim"]) == (N_IMAGES[e], N_IMAGES[e], e)
    assert math.isfinite(want) and want > 1e-3                               # two different sets
    assert abs(got["frechet_distance"] - want) <= TOLERANCE[e]
    # a spread is tr(cov) = (tr G - s.s / n) / (n - 1): the moments bound carried through, plus the roundings of that line
    # (terms up to tr G = n for unit-norm rows)
    for key, x, cov in (("spread_real", c["emb"][0], cov_r), ("spread_generated", c["emb"][1], cov_f)):
        bs, bg = moments_bound(x)
        n = x.shape[0]
        bound = (np.trace(bg) + 2 * float(np.abs(x.sum(axis=0)) @ bs) / n + 8 * U2 * n) / (n - 1)
        print(f"E={e} {key}: {got[key]!r} host {np.trace(cov)!r} bound {bound:.3e}")
        assert abs(got[key] - np.trace(cov)) <= bound and 0 < got[key] <= 1.0 + 1.0 / (n - 1)
    # the CNNEncoder module alone gives the same embeddings: the same chunks, the same figures bit for bit
    enc = calculate_verifier_frechet_distance(c["real"], c["fake"], c["model"].encoder.eval(), max_batch=40)
    assert enc == got


@pytest.mark.parametrize("e", [40, 128])
def test_a_set_against_itself(e):
    from signature_gan_amd.utils.metrics import calculate_verifier_frechet_distance
    c = case(e)
    got = calculate_verifier_frechet_distance(c["real"], c["real"], c["model"])
    print(f"E={e}: self distance {got['frechet_distance']:.3e} tolerance {TOLERANCE[e]:.3e}")
    assert abs(got["frechet_distance"]) <= TOLERANCE[e]
    assert got["spread_real"] == got["spread_generated"]
    with pytest.raises(ValueError, match="at least 2"):
        calculate_verifier_frechet_distance(c["real"][:1], c["real"], c["model"])


def test_evaluate_cli_with_a_verifier(tmp_path, capsys):
    """A tiny Generator checkpoint, a verifier checkpoint, 40 samples at batch 16 and 12 PNGs: with the flag the report
    holds the distance and both spreads, without it not one verifier key, and without real images the reason."""
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

    with_flag, text = run("a", "--real_dir", str(real_dir), "--verifier_checkpoint", str(vck))
    m = with_flag["metrics"]
    assert m["verifier_checkpoint"] == str(vck) and "verifier_frechet_error" not in m
    assert math.isfinite(m["verifier_frechet_distance"]) and m["verifier_frechet_distance"] > 0
    assert set(m["verifier_embedding_spread"]) == {"generated", "real"}
    assert all(0 < v <= 1 for v in m["verifier_embedding_spread"].values())
    assert with_flag["summary"]["verifier_frechet_distance"] == m["verifier_frechet_distance"]
    assert f"Verifier Frechet Distance: {m['verifier_frechet_distance']:.4f} (lower is better)" in text

    plain, text = run("b", "--real_dir", str(real_dir))
    assert not [k for k in plain["metrics"] if k.startswith("verifier")] and "verifier_frechet_distance" not in plain["summary"]
    assert "erifier" not in text
    # the flag changes nothing else: the same seed's samples, the same statistics
    for key in ("stroke_density", "foreground_ratio", "real_stroke_density", "real_foreground_ratio", "fid_score", "lpips_diversity"):
        assert plain["metrics"][key] == m[key], key

    no_real, text = run("c", "--verifier_checkpoint", str(vck))
    assert no_real["metrics"]["verifier_frechet_distance"] is None
    assert no_real["metrics"]["verifier_frechet_error"] == "no real images provided"
    assert no_real["summary"]["verifier_frechet_distance"] is None
    assert "Verifier Frechet Distance: Not computed - no real images provided" in text

    unreadable, _ = run("d", "--real_dir", str(real_dir), "--verifier_checkpoint", str(tmp_path / "none.pth"))
    assert unreadable["metrics"]["verifier_frechet_distance"] is None
    assert "Checkpoint not found" in unreadable["metrics"]["verifier_frechet_error"]


if __name__ == "__main__":
    for e_ in (40, 128):
        d_, t_, w_ = cpu_sensitivity(e_)
        print(f"E = {e_}, n = {N_IMAGES[e_]}: distance {d_:.4f}, traces {t_:.4f}, largest change {w_:.3e} ({w_ / t_:.2e} of the traces)")
