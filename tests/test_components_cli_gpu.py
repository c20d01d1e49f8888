"""The two CLIs' component flags on the MI355X, on a tiny randomly initialised checkpoint the test writes:
``evaluate_vanilla_gan_signatures --components`` and ``generate_signatures --despeckle``.  The yardstick is scipy
(componentscommon.yardstick) on the bytes the runs themselves produce; every comparison is exact.

The networks are reference_init's under a fixed seed with the two gains of tests/test_realism_filter_gpu.py: the Generator's
final conv times 1024 (bytes on both sides of 128, so there is ink and there are specks) and the Discriminator's classifier
weight times 1024 (scores that differ)."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import componentscommon as CC

pytestmark = pytest.mark.gpu

LATENT, N, BATCH, SEEDV, MIN_AREA = 100, 10, 4, 77, 6


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
def checkpoint(nets, tmp_path_factory):
    g, d = nets
    ck = tmp_path_factory.mktemp("components_cli") / "checkpoint.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": 64}}, ck)
    return ck


def read_pngs(folder, prefix, n):
    return [np.array(Image.open(os.path.join(folder, f"{prefix}_{i + 1:06d}.png")).convert("L")) for i in range(n)]


def file_bytes(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


def generate(checkpoint, out, *flags):
    from signature_gan_amd import generate_signatures as cli
    cli.main(["--checkpoint", str(checkpoint), "--n_samples", str(N), "--output_dir", str(out), "--batch_size", str(BATCH),
              "--seed", str(SEEDV), "--prefix", "sig", *flags])


def yardstick_sum(images, threshold=128):
    stats = np.stack([CC.yardstick(im, threshold, 8, MIN_AREA, 255)[0] for im in images]).astype(np.int64)
    return int(stats[:, CC.SMALL_COMPONENTS].sum()), int(stats[:, CC.SMALL_INK].sum())


def test_plain_generation_is_unchanged_without_the_flag_and_cleaned_with_it(checkpoint, tmp_path):
    generate(checkpoint, tmp_path / "a")
    generate(checkpoint, tmp_path / "b")
    a, b = file_bytes(tmp_path / "a"), file_bytes(tmp_path / "b")
    assert a == b and sorted(a) == [f"sig_{i + 1:06d}.png" for i in range(N)]          # no new file, the same bytes
    generate(checkpoint, tmp_path / "c", "--despeckle", str(MIN_AREA))
    raw, clean = read_pngs(tmp_path / "a", "sig", N), read_pngs(tmp_path / "c", "sig", N)
    want = [CC.yardstick(im, 128, 8, MIN_AREA, 255)[2] for im in raw]
    assert all(np.array_equal(c, w) for c, w in zip(clean, want))
    assert any(not np.array_equal(c, r) for c, r in zip(clean, raw)), "the random Generator drew no speck: the test shows nothing"
    report = json.load(open(tmp_path / "c" / "sig_despeckle.json"))["despeckle"]
    comps, pixels = yardstick_sum(raw)
    assert report == {"min_area": MIN_AREA, "threshold": 128, "connectivity": 8, "removed_components": comps, "removed_pixels": pixels}
    assert sum(int((c != r).sum()) for c, r in zip(clean, raw)) == pixels               # a speck's byte is < 128, fill is 255
    # the default minimum area, and --threshold's binarisation on top of a cleaning at that threshold
    generate(checkpoint, tmp_path / "d", "--despeckle")
    assert json.load(open(tmp_path / "d" / "sig_despeckle.json"))["despeckle"]["min_area"] == 4
    assert all(np.array_equal(c, CC.yardstick(r, 128, 8, 4, 255)[2]) for c, r in zip(read_pngs(tmp_path / "d", "sig", N), raw))
    generate(checkpoint, tmp_path / "e", "--despeckle", str(MIN_AREA), "--threshold", "100")
    for got, r in zip(read_pngs(tmp_path / "e", "sig", N), raw):
        assert np.array_equal(got, np.where(CC.yardstick(r, 100, 8, MIN_AREA, 255)[2] < 100, 0, 255))


@pytest.mark.parametrize("threshold", [None, 127])
def test_filtered_generation_scores_the_cleaned_bytes(nets, checkpoint, tmp_path, threshold):
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d = nets
    extra = [] if threshold is None else ["--threshold", str(threshold)]
    generate(checkpoint, tmp_path / "plain", "--filter_by_realism", "--oversampling_ratio", "2.5", *extra)
    generate(checkpoint, tmp_path / "plain2", "--filter_by_realism", "--oversampling_ratio", "2.5", *extra)
    assert file_bytes(tmp_path / "plain") == file_bytes(tmp_path / "plain2")
    assert isinstance(json.load(open(tmp_path / "plain" / "sig_scores.json")), list)    # the bare list, as before
    generate(checkpoint, tmp_path / "clean", "--filter_by_realism", "--oversampling_ratio", "2.5", "--despeckle", str(MIN_AREA), *extra)
    doc = json.load(open(tmp_path / "clean" / "sig_scores.json"))
    written = read_pngs(tmp_path / "clean", "sig", N)
    assert [r["file"] for r in doc["records"]] == [f"sig_{i + 1:06d}.png" for i in range(N)]
    # the undespeckled pool (25 images, the same seeds and batches), cleaned by the yardstick, scored by d_score_u8 in the
    # run's own batches (the Discriminator's kernels are chosen by batch size, so its last bits are a batch's)
    pool, _ = generate_signatures_filtered(g, d, 25, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH, oversampling_ratio=1.0)
    assert len(pool) == 25
    raw = sorted((np.array(im) for im in pool), key=lambda a: a.tobytes())
    # generation order is lost in the ranked pool: regenerate it batch by batch as the run does
    from signature_gan_amd.utils.inference import _seed_batch, filter_plan
    ordered = []
    for b, batch_seed in filter_plan(N, 2.5, BATCH, SEEDV)[1]:
        _seed_batch(batch_seed)
        ordered += list(g._engine.g_generate_u8(torch.randn(b, LATENT, device="cuda")).cpu().numpy())
    assert [a.tobytes() for a in sorted(ordered, key=lambda a: a.tobytes())] == [a.tobytes() for a in raw]
    ink = 128 if threshold is None else threshold
    cleaned = [CC.yardstick(im, ink, 8, MIN_AREA, 255) for im in ordered]
    pool_scores = []
    for i in range(0, 25, BATCH):
        batch = torch.from_numpy(np.stack([c[2] for c in cleaned[i:i + BATCH]])).to("cuda")
        pool_scores += [float(v) for v in d.score_u8(batch, binarize=threshold).cpu()]
    rank = sorted(range(25), key=lambda i: pool_scores[i], reverse=True)[:N]            # stable: ties in generation order
    assert [r["score"] for r in doc["records"]] == [pool_scores[i] for i in rank]
    for w, i in zip(written, rank):
        final = cleaned[i][2] if threshold is None else np.where(cleaned[i][2] < threshold, 0, 255).astype(np.uint8)
        assert np.array_equal(w, final)
    stats = np.stack([cleaned[i][0] for i in rank]).astype(np.int64)
    assert doc["despeckle"] == {"min_area": MIN_AREA, "threshold": ink, "connectivity": 8,
                                "removed_components": int(stats[:, CC.SMALL_COMPONENTS].sum()),
                                "removed_pixels": int(stats[:, CC.SMALL_INK].sum())}
    assert doc["despeckle"]["removed_components"] > 0
    # the host route (what a train-mode network falls back to) gives the same images and scores
    from signature_gan_amd.utils.inference import Despeckle
    images, host_scores = generate_signatures_filtered(g, d, N, LATENT, torch.device("cuda"), seed=SEEDV, batch_size=BATCH,
                                                       oversampling_ratio=2.5, threshold=threshold, route="host",
                                                       despeckle=Despeckle(MIN_AREA, ink))
    assert host_scores == [r["score"] for r in doc["records"]]
    assert all(np.array_equal(np.array(im), w) for im, w in zip(images, written))


def test_refined_generation_is_cleaned_and_reports(checkpoint, tmp_path):
    generate(checkpoint, tmp_path / "r0", "--refine_by_realism", "--refine_steps", "2")
    generate(checkpoint, tmp_path / "r1", "--refine_by_realism", "--refine_steps", "2", "--despeckle", str(MIN_AREA))
    raw, clean = read_pngs(tmp_path / "r0", "sig", N), read_pngs(tmp_path / "r1", "sig", N)
    assert all(np.array_equal(c, CC.yardstick(r, 128, 8, MIN_AREA, 255)[2]) for c, r in zip(clean, raw))
    before, after = json.load(open(tmp_path / "r0" / "sig_refine.json")), json.load(open(tmp_path / "r1" / "sig_refine.json"))
    assert isinstance(before, list) and after["records"] == before
    comps, pixels = yardstick_sum(raw)
    assert (after["despeckle"]["removed_components"], after["despeckle"]["removed_pixels"]) == (comps, pixels)


def test_adapted_generation_is_cleaned_and_reports(checkpoint, tmp_path):
    src = tmp_path / "targets"
    src.mkdir()
    fam = CC.families(64, 64)
    for name in ("strokes", "strokes_2"):
        Image.fromarray(fam[name], mode="L").save(src / f"{name}.png")
    flags = ["--adapt", str(src), "--adapt_steps", "2", "--project_steps", "4"]
    generate(checkpoint, tmp_path / "a0", *flags)
    generate(checkpoint, tmp_path / "a1", *flags, "--despeckle", str(MIN_AREA))
    raw, clean = read_pngs(tmp_path / "a0", "sig", N), read_pngs(tmp_path / "a1", "sig", N)
    assert all(np.array_equal(c, CC.yardstick(r, 128, 8, MIN_AREA, 255)[2]) for c, r in zip(clean, raw))
    before, after = json.load(open(tmp_path / "a0" / "sig_adapt.json")), json.load(open(tmp_path / "a1" / "sig_adapt.json"))
    comps, pixels = yardstick_sum(raw)
    assert "despeckle" not in before
    assert after.pop("despeckle") == {"min_area": MIN_AREA, "threshold": 128, "connectivity": 8, "removed_components": comps,
                                      "removed_pixels": pixels}
    assert after == before


class _Recorder:
    def __init__(self):
        self.batches = []

    def update(self, u8):
        self.batches.append(u8.cpu().numpy().copy())


def test_evaluate_reports_fragmentation_equal_to_scipy(checkpoint, tmp_path):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd.data_loader_signatures import SignatureDataset
    from signature_gan_amd.utils.metrics import fragmentation_from_counters
    real_dir = tmp_path / "real"
    real_dir.mkdir()
    for i, (name, img) in enumerate(CC.families(64, 64).items()):
        Image.fromarray(img, mode="L").save(real_dir / f"{i:02d}_{name}.png")
    common = ["--checkpoint", str(checkpoint), "--n_samples", "22", "--batch_size", "8", "--seed", "5", "--n_grids", "0", "--real_dir", str(real_dir)]

    def run(out, *flags):
        assert ev.main(common + ["--output_dir", str(out), *flags]) == 0
        (path,) = glob.glob(str(out / "evaluation_report_*.json"))
        return json.load(open(path))

    plain, plain2 = run(tmp_path / "p1"), run(tmp_path / "p2")
    drop = lambda m: {k: v for k, v in m.items() if k != "metrics_computed_at"}      # noqa: E731
    assert "fragmentation" not in plain["metrics"] and drop(plain["metrics"]) == drop(plain2["metrics"])
    assert plain["summary"] == plain2["summary"]
    with_flag = run(tmp_path / "c", "--components", str(MIN_AREA))
    frag = with_flag["metrics"].pop("fragmentation")
    assert drop(with_flag["metrics"]) == drop(plain["metrics"])                       # every other number is what it was
    # the bytes the run generated: the same seed, the same loading, the same batches
    torch.manual_seed(5); np.random.seed(5)
    generator, _ = ev.load_generator_from_checkpoint(checkpoint, torch.device("cuda"))
    rec = _Recorder()
    ev.generate_samples(generator, 22, generator.latent_dim, torch.device("cuda"), 8, keep_images=0, component_sink=rec)
    fake = np.concatenate(rec.batches)
    assert fake.shape == (22, 64, 64)
    want = fragmentation_from_counters(np.stack([CC.yardstick(im, 128, 8, MIN_AREA, 255)[0] for im in fake]))
    assert frag["generated"] == want and want["n"] == 22 and want["components_mean"] > 0
    ds = SignatureDataset(real_dir)
    real = [ds.decode(i, 64) for i in range(len(ds))]
    assert frag["real"] == fragmentation_from_counters(np.stack([CC.yardstick(im, 128, 8, MIN_AREA, 255)[0] for im in real]))
    assert (frag["threshold"], frag["connectivity"], frag["min_area"]) == (128, 8, MIN_AREA)
    # without a real directory the real side is omitted; the default minimum area
    out = tmp_path / "n"
    assert ev.main(["--checkpoint", str(checkpoint), "--n_samples", "6", "--batch_size", "8", "--seed", "5", "--n_grids", "0",
                    "--output_dir", str(out), "--components"]) == 0
    (path,) = glob.glob(str(out / "evaluation_report_*.json"))
    frag = json.load(open(path))["metrics"]["fragmentation"]
    assert "real" not in frag and frag["min_area"] == 4 and frag["generated"]["n"] == 6


def test_calculate_fragmentation_takes_bytes_and_fp32(nets):
    from signature_gan_amd.utils.metrics import calculate_fragmentation, fragmentation_from_counters
    g, _ = nets
    torch.manual_seed(3)
    z = torch.randn(6, LATENT, device="cuda")
    u8, _, f32 = g._engine.g_generate_u8(z, threshold=0.5, want_f32=True)
    want = fragmentation_from_counters(np.stack([CC.yardstick(im, 128, 8, 4, 255)[0] for im in u8.cpu().numpy()]))
    assert calculate_fragmentation(u8) == want
    assert calculate_fragmentation(f32) == want                                      # quantised by the generation rule
    assert calculate_fragmentation(f32.cpu()) == want
    assert calculate_fragmentation(u8, min_area=9, connectivity=4) == fragmentation_from_counters(
        np.stack([CC.yardstick(im, 128, 4, 9, 255)[0] for im in u8.cpu().numpy()]))
