"""``generate_signatures --filter_by_realism --diverse`` on the MI355X, on tiny randomly initialised checkpoints the test writes
(the networks of tests/test_realism_filter_gpu.py, the E = 40 verifier of verifiercommon): which files appear, that every PNG
holds the pool row the report names, the report's keys, --diverse_existing_dir / --diverse_min_separation including a run that
selects fewer than asked, and that a run without --diverse writes exactly the files it wrote before."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import verifiercommon as VC

pytestmark = pytest.mark.gpu

LATENT, N, BATCH, SEEDV, RATIO, E = 100, 6, 16, 77, 4.0, 40
REPORT_KEYS = {"pool", "eligible", "requested", "selected", "stopped_by", "picks", "coverage_radius", "diverse", "top_n"}
PICK_KEYS = {"pool_index", "realism", "gain", "nearest_real", "file"}
STAT_KEYS = {"min_nn_distance", "mean_nn_distance", "mean_realism"}


@pytest.fixture(scope="module")
def nets():
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=LATENT, output_size=64).to("cuda").eval()
    d = Discriminator(input_size=64).to("cuda").eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
        d.state_dict()["classifier.0.weight"].mul_(1024.0)
    g._engine.params_changed(); d._engine.params_changed()
    return g, d


@pytest.fixture(scope="module")
def checkpoints(nets, tmp_path_factory):
    g, d = nets
    folder = tmp_path_factory.mktemp("diverse_cli")
    ck, vk = folder / "checkpoint.pth", folder / "verifier.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": 64}}, ck)
    torch.save({"model_state_dict": VC.torch_state(E), "embedding_dim": E, "epoch": 1}, vk)
    return ck, vk


@pytest.fixture(scope="module")
def pool(nets):
    """The 24 pool images in generation order, as the run draws them."""
    from signature_gan_amd.utils.inference import _seed_batch, filter_plan
    g, _ = nets
    out = []
    for b, batch_seed in filter_plan(N, RATIO, BATCH, SEEDV)[1]:
        _seed_batch(batch_seed)
        out += list(g._engine.g_generate_u8(torch.randn(b, LATENT, device="cuda")).cpu().numpy())
    return out


def generate(checkpoints, out, *flags, diverse=True):
    from signature_gan_amd import generate_signatures as cli
    ck, vk = checkpoints
    extra = ["--diverse", "--verifier_checkpoint", str(vk)] if diverse else []
    cli.main(["--checkpoint", str(ck), "--n_samples", str(N), "--output_dir", str(out), "--batch_size", str(BATCH), "--seed", str(SEEDV),
              "--prefix", "sig", "--filter_by_realism", "--oversampling_ratio", str(RATIO), *extra, *flags])


def check_run(out, pool, threshold=None):
    report = json.load(open(os.path.join(out, "sig_diverse.json")))
    scores = json.load(open(os.path.join(out, "sig_scores.json")))
    assert set(report) == REPORT_KEYS and set(report["diverse"]) == set(report["top_n"]) == STAT_KEYS
    n = report["selected"]
    names = [f"sig_{i + 1:06d}.png" for i in range(n)]
    assert sorted(os.listdir(out)) == sorted(names + ["sig_scores.json", "sig_diverse.json"])
    assert len(report["picks"]) == n and all(set(p) == PICK_KEYS for p in report["picks"])
    assert [p["file"] for p in report["picks"]] == names == [r["file"] for r in scores]
    assert [p["realism"] for p in report["picks"]] == [r["score"] for r in scores]
    assert len({p["pool_index"] for p in report["picks"]}) == n and report["pool"] == len(pool) and report["requested"] == N
    for p in report["picks"]:
        want = pool[p["pool_index"]]
        img = Image.open(os.path.join(out, p["file"]))
        if threshold is not None:
            assert img.mode == "1"
            want = np.where(want < threshold, 0, 255).astype(np.uint8)
        assert np.array_equal(np.array(img.convert("L")), want)
    return report


def test_diverse_run_writes_the_picked_pool_rows(checkpoints, pool, tmp_path, capsys):
    generate(checkpoints, tmp_path / "a")
    report = check_run(tmp_path / "a", pool)
    assert (report["selected"], report["eligible"], report["stopped_by"]) == (N, 12, "count")       # --diverse_keep_ratio 0.5 of 24
    assert report["picks"][0]["gain"] is None and all(p["gain"] > 0 for p in report["picks"][1:])
    assert report["picks"][0]["realism"] == max(p["realism"] for p in report["picks"])                # the first pick: the best score
    assert all(p["nearest_real"] is None for p in report["picks"]) and report["coverage_radius"] > 0
    assert "Mean realism" in capsys.readouterr().out
    generate(checkpoints, tmp_path / "b", "--threshold", "127", "--diverse_keep_ratio", "1.0")
    report = check_run(tmp_path / "b", pool, threshold=127)
    assert report["eligible"] == 24


def test_existing_set_and_min_separation(checkpoints, pool, tmp_path, capsys):
    generate(checkpoints, tmp_path / "first", "--diverse_keep_ratio", "1.0")
    first = check_run(tmp_path / "first", pool)
    existing = tmp_path / "existing"
    existing.mkdir()
    taken = [p["pool_index"] for p in first["picks"][:3]]
    for i in taken:
        Image.fromarray(pool[i], mode="L").save(existing / f"old_{i:02d}.png")
    # a second run against the same pool keeps away from what the first one kept: those rows are at distance 0 from the set
    generate(checkpoints, tmp_path / "second", "--diverse_keep_ratio", "1.0", "--diverse_existing_dir", str(existing),
             "--diverse_min_separation", "1e-6")
    second = check_run(tmp_path / "second", pool)
    assert not set(taken) & {p["pool_index"] for p in second["picks"]} and second["selected"] == N
    assert all(p["gain"] is not None and p["gain"] >= 1e-6 for p in second["picks"])                 # anchors: no +inf first pick
    gains = [p["gain"] for p in second["picks"]]
    assert all(a >= b for a, b in zip(gains, gains[1:]))
    # a separation between two of those gains: the run stops early, says so and still succeeds
    sep = 0.5 * (gains[2] + gains[3])
    assert gains[2] > sep > gains[3]
    capsys.readouterr()
    generate(checkpoints, tmp_path / "third", "--diverse_keep_ratio", "1.0", "--diverse_existing_dir", str(existing),
             "--diverse_min_separation", repr(sep))
    third = check_run(tmp_path / "third", pool)
    assert third["selected"] == 3 and third["stopped_by"] == "separation" and third["picks"] == second["picks"][:3]
    assert f"Selected 3 of the {N} signatures asked for" in capsys.readouterr().out


def test_real_dir_bars_a_copy(checkpoints, pool, tmp_path):
    generate(checkpoints, tmp_path / "free", "--diverse_keep_ratio", "1.0")
    victim = check_run(tmp_path / "free", pool)["picks"][1]["pool_index"]
    real = tmp_path / "real"
    real.mkdir()
    rng = np.random.default_rng(3)
    for i in range(5):
        Image.fromarray(rng.integers(0, 256, size=(64, 64), dtype=np.uint8), mode="L").save(real / f"r{i}.png")
    Image.fromarray(pool[victim], mode="L").save(real / "copy.png")
    generate(checkpoints, tmp_path / "barred", "--diverse_keep_ratio", "1.0", "--diverse_real_dir", str(real),
             "--diverse_memorisation_ratio", "0.01")
    report = check_run(tmp_path / "barred", pool)
    assert victim not in [p["pool_index"] for p in report["picks"]] and report["eligible"] < 24
    assert all(p["nearest_real"] > 0 for p in report["picks"])


def test_run_without_the_flag_writes_what_it_wrote(checkpoints, nets, tmp_path):
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    generate(checkpoints, tmp_path / "p1", diverse=False)
    generate(checkpoints, tmp_path / "p2", diverse=False)
    files = lambda folder: {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}      # noqa: E731
    a, b = files(tmp_path / "p1"), files(tmp_path / "p2")
    names = [f"sig_{i + 1:06d}.png" for i in range(N)]
    assert a == b and sorted(a) == sorted(names + ["sig_scores.json"])                                # no sig_diverse.json
    images, scores = generate_signatures_filtered(g, d, N, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH,
                                                  oversampling_ratio=RATIO, route="host")
    records = json.loads(a["sig_scores.json"])
    assert [r["file"] for r in records] == names and [r["score"] for r in records] == scores
    for name, want in zip(names, images):
        assert np.array_equal(np.array(Image.open(tmp_path / "p1" / name)), np.array(want))


def test_despeckle_composes(checkpoints, pool, tmp_path):
    """--despeckle cleans the pool before it is scored and embedded: every PNG is the cleaned pool row the report names, and
    sig_scores.json takes the shape it has under --despeckle elsewhere."""
    from signature_gan_amd.components import despeckle_u8
    generate(checkpoints, tmp_path / "c", "--despeckle", "6", "--diverse_keep_ratio", "1.0")
    report = json.load(open(tmp_path / "c" / "sig_diverse.json"))
    doc = json.load(open(tmp_path / "c" / "sig_scores.json"))
    assert set(doc) == {"despeckle", "records"} and doc["despeckle"]["min_area"] == 6 and len(doc["records"]) == N == report["selected"]
    cleaned = despeckle_u8(torch.from_numpy(np.stack(pool)).to("cuda"), 128, 8, 6, 255).cpu().numpy()
    assert any(not np.array_equal(c, r) for c, r in zip(cleaned, pool)), "no speck in the pool: the test shows nothing"
    for p, rec in zip(report["picks"], doc["records"]):
        assert p["file"] == rec["file"] and p["realism"] == rec["score"]
        assert np.array_equal(np.array(Image.open(tmp_path / "c" / p["file"])), cleaned[p["pool_index"]])
