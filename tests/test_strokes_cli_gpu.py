"""The two CLIs' stroke flags on the MI355X, on a tiny randomly initialised checkpoint the test writes:
``evaluate_vanilla_gan_signatures --strokes`` and ``generate_signatures --pen_width``.  The yardstick is the numpy restatement
(strokescommon.reference) on the bytes the runs themselves produce; every comparison is exact.

The networks are reference_init's under a fixed seed with the two gains of tests/test_components_cli_gpu.py: the Generator's
final conv times 1024 (bytes on both sides of 128, so there is ink) and the Discriminator's classifier weight times 1024."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import strokescommon as SC

pytestmark = pytest.mark.gpu

LATENT, N, BATCH, SEEDV = 100, 10, 4, 77


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
    ck = tmp_path_factory.mktemp("strokes_cli") / "checkpoint.pth"
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


def mean_width(images, threshold=128):
    hist = np.stack([SC.reference(im, threshold)[0][SC.WIDTH_HIST:] for im in images]).astype(np.int64).sum(axis=0)
    return float(int((hist * (2 * np.arange(1, 17) - 1)).sum()) / int(hist.sum()))


def test_pen_width_redraws_the_plain_runs_images(checkpoint, tmp_path):
    from signature_gan_amd import strokes
    generate(checkpoint, tmp_path / "a")
    generate(checkpoint, tmp_path / "b")
    a = file_bytes(tmp_path / "a")
    assert a == file_bytes(tmp_path / "b") and sorted(a) == [f"sig_{i + 1:06d}.png" for i in range(N)]       # no new file without the flag
    raw = read_pngs(tmp_path / "a", "sig", N)
    generate(checkpoint, tmp_path / "c", "--pen_width", "3")
    drawn = read_pngs(tmp_path / "c", "sig", N)
    made = strokes.restroke_u8(torch.from_numpy(np.stack(raw)).to("cuda"), strokes.radius2_for_pen_width(3)).cpu().numpy()
    assert all(np.array_equal(d, m) for d, m in zip(drawn, made))
    assert all(np.array_equal(d, SC.reference(r, 128, 1)[3]) for d, r in zip(drawn, raw))
    assert any(not np.array_equal(d, r) for d, r in zip(drawn, raw))
    report = json.load(open(tmp_path / "c" / "sig_pen_width.json"))
    assert report == {"pen_width": 3, "radius2": 1, "threshold": 128, "mean_width_before": mean_width(raw), "mean_width_after": mean_width(drawn)}
    assert sorted(os.listdir(tmp_path / "c")) == sorted(list(a) + ["sig_pen_width.json"])
    # --despeckle given as well runs first; --threshold is the ink threshold of both
    generate(checkpoint, tmp_path / "d", "--pen_width", "5", "--despeckle", "6", "--threshold", "100")
    import componentscommon as CC
    cleaned = [CC.yardstick(r, 100, 8, 6, 255)[2] for r in raw]
    assert all(np.array_equal(d, SC.reference(c, 100, 4)[3]) for d, c in zip(read_pngs(tmp_path / "d", "sig", N), cleaned))
    assert json.load(open(tmp_path / "d" / "sig_pen_width.json"))["mean_width_before"] == mean_width(cleaned, 100)
    assert os.path.exists(tmp_path / "d" / "sig_despeckle.json")


def test_generate_uint8_redraws_after_the_cleaning_and_the_host_route_equals_the_device_route(nets):
    from signature_gan_amd.utils.inference import Despeckle, PenWidth, generate_uint8
    import componentscommon as CC
    g, _ = nets
    torch.manual_seed(9)
    z = torch.randn(5, LATENT, device="cuda")
    raw = generate_uint8(g, z)
    assert (raw < 128).any() and (raw >= 128).any()
    pw = PenWidth(4)
    drawn = generate_uint8(g, z, Despeckle(6), pen_width=pw)
    cleaned = [CC.yardstick(r, 128, 8, 6, 255)[2] for r in raw]
    assert all(np.array_equal(d, SC.reference(c, 128, 2)[3]) for d, c in zip(drawn, cleaned))
    assert pw.report() == {"pen_width": 4, "radius2": 2, "threshold": 128, "mean_width_before": mean_width(cleaned),
                           "mean_width_after": mean_width(drawn)}
    # what a Generator left in train() mode takes: bytes on the host, redrawn through the device
    host = PenWidth(4)
    assert np.array_equal(host.redraw_host(np.stack(cleaned), z.device), drawn) and host.report() == pw.report()


class _Recorder:
    def __init__(self):
        self.batches = []

    def update(self, u8):
        self.batches.append(u8.cpu().numpy().copy())


def test_evaluate_reports_stroke_geometry_equal_to_the_restatement(checkpoint, tmp_path):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd.data_loader_signatures import SignatureDataset
    from signature_gan_amd.utils.metrics import calculate_stroke_geometry, stroke_geometry_from_counters
    real_dir = tmp_path / "real"
    real_dir.mkdir()
    for i, (name, img) in enumerate(SC.fills(64, 64).items()):
        Image.fromarray(img, mode="L").save(real_dir / f"{i:02d}_{name}.png")
    common = ["--checkpoint", str(checkpoint), "--n_samples", "22", "--batch_size", "8", "--seed", "5", "--n_grids", "0", "--real_dir", str(real_dir)]

    def run(out, *flags):
        assert ev.main(common + ["--output_dir", str(out), *flags]) == 0
        (path,) = glob.glob(str(out / "evaluation_report_*.json"))
        return json.load(open(path))

    plain = run(tmp_path / "p1")
    drop = lambda m: {k: v for k, v in m.items() if k != "metrics_computed_at"}      # noqa: E731
    assert "stroke_geometry" not in plain["metrics"]
    with_flag = run(tmp_path / "s", "--strokes")
    geo = with_flag["metrics"].pop("stroke_geometry")
    assert drop(with_flag["metrics"]) == drop(plain["metrics"]) and with_flag["summary"] == plain["summary"]
    # the bytes the run generated: the same seed, the same loading, the same batches
    torch.manual_seed(5); np.random.seed(5)
    generator, _ = ev.load_generator_from_checkpoint(checkpoint, torch.device("cuda"))
    rec = _Recorder()
    ev.generate_samples(generator, 22, generator.latent_dim, torch.device("cuda"), 8, keep_images=0, stroke_sink=rec)
    fake = np.concatenate(rec.batches)
    assert fake.shape == (22, 64, 64)
    want = stroke_geometry_from_counters(np.stack([SC.reference(im)[0] for im in fake]))
    assert geo["generated"] == want and want["images"] == 22 and want["mean_width"] is not None and want["bound_hit"] == 0
    assert geo["generated"] == calculate_stroke_geometry(torch.from_numpy(fake).to("cuda"))
    ds = SignatureDataset(real_dir)
    real = [ds.decode(i, 64) for i in range(len(ds))]
    assert geo["real"] == stroke_geometry_from_counters(np.stack([SC.reference(im)[0] for im in real]))
    assert geo["threshold"] == 128 and list(geo) == ["threshold", "generated", "real"]
    # without a real directory the real side is omitted
    out = tmp_path / "n"
    assert ev.main(["--checkpoint", str(checkpoint), "--n_samples", "6", "--batch_size", "8", "--seed", "5", "--n_grids", "0",
                    "--output_dir", str(out), "--strokes"]) == 0
    (path,) = glob.glob(str(out / "evaluation_report_*.json"))
    geo = json.load(open(path))["metrics"]["stroke_geometry"]
    assert "real" not in geo and geo["generated"]["images"] == 6


def test_calculate_stroke_geometry_takes_bytes_and_fp32(nets):
    from signature_gan_amd.utils.metrics import calculate_stroke_geometry, stroke_geometry_from_counters
    g, _ = nets
    torch.manual_seed(3)
    z = torch.randn(6, LATENT, device="cuda")
    u8, _, f32 = g._engine.g_generate_u8(z, threshold=0.5, want_f32=True)
    want = stroke_geometry_from_counters(np.stack([SC.reference(im)[0] for im in u8.cpu().numpy()]))
    assert calculate_stroke_geometry(u8) == want
    assert calculate_stroke_geometry(f32) == want                                    # quantised by the generation rule
    assert calculate_stroke_geometry(f32.cpu()) == want
    assert calculate_stroke_geometry(u8, threshold=100) == stroke_geometry_from_counters(
        np.stack([SC.reference(im, 100)[0] for im in u8.cpu().numpy()]))
