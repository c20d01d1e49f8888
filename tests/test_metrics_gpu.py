"""siggan_image_stats, utils/metrics.py and the evaluation CLI on the device, each held exactly to a restatement on the CPU
(numpy float32 counts; the reference's statistics formula with torch)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from common import I, O, SEED
from strokecommon import foreground_dict, numpy_counts, stroke_dict, torch_densities

pytestmark = pytest.mark.gpu


# (3, 4096): aligned rows, one block per image.  (2, 4099): the second row starts three floats past a 16-byte boundary (a
# scalar head) and both rows end in a scalar tail.  (2, 24581): four blocks per image, head and tail again.
@pytest.mark.parametrize("shape", [(3, 4096), (2, 4099), (2, 3 * 8192 + 5)])
@pytest.mark.parametrize("thr", [0.5, 0.6])
def test_image_stats_counts(shape, thr):
    from signature_gan_amd.engine import Engine
    gen = torch.Generator().manual_seed(shape[1])
    x = torch.rand(shape, generator=gen) * 2 - 1
    # the values on which a comparison can go wrong, at both ends and in the middle of every row: the two zeros, the range's
    # ends, and the signed branch's boundary 2 thr - 1 with its two fp32 neighbours ((t + 1) * 0.5 < thr turns there)
    edge = np.float32(2) * np.float32(thr) - np.float32(1)
    planted = [0.0, -0.0, 1.0, -1.0, float(edge), float(np.nextafter(edge, np.float32(-2))), float(np.nextafter(edge, np.float32(2))),
               float(np.float32(thr)), float(np.nextafter(np.float32(thr), np.float32(-2)))]
    p = shape[1]
    for b in range(shape[0]):
        for start in (0, p // 2 - 3, p - len(planted)):
            x[b, start:start + len(planted)] = torch.tensor(planted)
    got = Engine.image_stats(x.cuda(), thr).cpu().numpy()
    want = numpy_counts(x.numpy(), thr)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)
    assert (want[:, 0] > 0).all() and (want[:, 1] != want[:, 2]).all()      # the three counters tell different things here


def test_image_stats_without_negatives_and_refusals():
    from signature_gan_amd.engine import Engine
    x = torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(1))
    x[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 0.5, 1.0])
    got = Engine.image_stats(x.cuda(), 0.5).cpu().numpy()
    assert np.array_equal(got, numpy_counts(x.numpy(), 0.5)) and (got[:, 0] == 0).all()
    sliced = x.cuda()[:, :, :, 1:]                         # rows of 31 floats at odd offsets, made contiguous by the caller
    assert np.array_equal(Engine.image_stats(sliced.contiguous(), 0.5).cpu().numpy(), numpy_counts(sliced.cpu().numpy(), 0.5))
    with pytest.raises(ValueError):
        Engine.image_stats(sliced, 0.5)                    # not contiguous
    with pytest.raises(ValueError):
        Engine.image_stats(x.cuda().double(), 0.5)
    with pytest.raises(ValueError):
        Engine.image_stats(x.cuda(), float("nan"))
    with pytest.raises(ValueError):
        Engine.image_stats(torch.empty(0, 16, device="cuda"), 0.5)


def _grid_values(shape, signed, seed):
    """Values (2k + 1) / 128 in (0, 1) (or mapped to (-1, 1)): channel means are exact in fp32 on either device and never
    land on the threshold, so the device's mean and the CPU's cannot disagree about a pixel."""
    k = torch.randint(0, 64, shape, generator=torch.Generator().manual_seed(seed))
    x = (2 * k + 1).float() / 128
    return x * 2 - 1 if signed else x


@pytest.mark.parametrize("kind", ["signed", "unit", "three_channel", "cpu_tensor"])
def test_stroke_density_and_foreground_ratio(kind):
    from signature_gan_amd.utils.metrics import calculate_foreground_ratio, calculate_stroke_density
    gen = torch.Generator().manual_seed(7)
    if kind == "signed":
        x = torch.rand(6, 1, 64, 64, generator=gen) * 2 - 1
    elif kind == "unit":
        x = torch.rand(6, 1, 64, 64, generator=gen)
    elif kind == "three_channel":
        x = _grid_values((5, 3, 32, 32), True, 3)
    else:
        x = torch.rand(4, 1, 32, 32, generator=gen) * 2 - 1
    dev = x if kind == "cpu_tensor" else x.cuda()          # a CPU tensor is moved to the device
    for thr in (0.5, 0.4):
        want = torch_densities(x, thr)
        assert want.min() > 0 and want.max() < 1
        assert calculate_stroke_density(dev, threshold=thr) == stroke_dict(want)
        assert calculate_foreground_ratio(dev, threshold=thr) == foreground_dict(want)
    assert calculate_stroke_density(dev) == stroke_dict(torch_densities(x, 0.5))      # the default threshold


def test_evaluate_cli_end_to_end(tmp_path, capsys):
    """Checkpoint of an engine-backed Generator in, report out: the statistics equal the CPU formula on the same seed's
    images regenerated with g_forward, the real folder's on the loader's decode + byte table."""
    from PIL import Image
    from signature_gan_amd import evaluate_vanilla_gan_signatures as cli
    from signature_gan_amd.data_loader_signatures import SignatureDataset, normalize_lut
    from signature_gan_amd.generator_vanilla_gan import Generator
    from signature_gan_amd.utils.inference import load_generator
    size, latent, n, bs, seed = 64, 100, 70, 32, 3
    g = Generator(latent_dim=latent, output_size=size).to("cuda")
    g.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in I.gen_state(O.g_state_specs(latent, size), SEED["state_g"]).items()})
    ck = tmp_path / "ck.pt"
    torch.save({"epoch": 2, "generator_state_dict": {k: v.detach().cpu().clone() for k, v in g.state_dict().items()},
                "config": {"latent_dim": latent, "image_size": size, "current_epoch": 2}}, ck)
    real_dir, out_dir = tmp_path / "real", tmp_path / "out"
    real_dir.mkdir()
    rng = np.random.default_rng(0)
    for i in range(12):
        Image.fromarray(rng.integers(0, 256, (40, 52), dtype=np.uint8), "L").save(real_dir / f"r{i:02d}.png")

    rc = cli.main(["--checkpoint", str(ck), "--n_samples", str(n), "--batch_size", str(bs), "--n_grids", "1", "--grid_size", "16",
                   "--seed", str(seed), "--real_dir", str(real_dir), "--output_dir", str(out_dir)])
    text = capsys.readouterr().out
    assert rc == 0, text
    for line in (f"Random seed set to: {seed}", f"Generating {n} samples...", f"  Generated {n}/{n} samples", "Loading 12 real images from",
                 "EVALUATION SUMMARY", "--- Comparison with Real Images ---",
                 "Evaluation complete!"):
        assert line in text, line
    reports, grids = glob.glob(str(out_dir / "evaluation_report_*.json")), glob.glob(str(out_dir / "sample_grid_*_1.png"))
    assert len(reports) == 1 and len(grids) == 1
    assert Image.open(grids[0]).size == (4 * (size + 2) + 2,) * 2              # 16 samples, 4 per row, padding 2
    with open(reports[0]) as f:
        rep = json.load(f)
    assert set(rep) == {"evaluation_info", "model_config", "metrics", "summary"}
    assert set(rep["evaluation_info"]) == {"checkpoint", "evaluation_timestamp", "sample_grids"}
    assert rep["evaluation_info"]["sample_grids"] == grids and rep["model_config"]["image_size"] == size
    assert set(rep["summary"]) == {"fid_score", "lpips_diversity", "stroke_density_mean", "foreground_ratio_mean", "n_samples_evaluated"}
    m = rep["metrics"]
    assert m["n_samples"] == n and m["image_shape"] == [1, size, size] and rep["summary"]["n_samples_evaluated"] == n
    assert m["fid_score"] is None and m["fid_error"] and m["lpips_diversity"] is None and m["lpips_error"]

    # the same seed's images, as the CLI draws them: seed, load the Generator, then one randn per batch
    torch.manual_seed(seed)
    g2, _ = load_generator(str(ck), torch.device("cuda"))
    imgs = torch.cat([g2(torch.randn(min(bs, n - i), latent, device="cuda")).cpu() for i in range(0, n, bs)])
    want = torch_densities(imgs, 0.5)
    assert want.max() > want.min() > 0
    assert m["stroke_density"] == stroke_dict(want) and m["foreground_ratio"] == foreground_dict(want)
    assert rep["summary"]["stroke_density_mean"] == stroke_dict(want)["mean"]

    ds = SignatureDataset(real_dir)
    real = normalize_lut((-1.0, 1.0))[torch.from_numpy(np.stack([ds.decode(i, size) for i in range(12)])).long()].unsqueeze(1)
    want_real = torch_densities(real, 0.5)
    assert m["real_stroke_density"] == stroke_dict(want_real) and m["real_foreground_ratio"] == foreground_dict(want_real)
    assert os.path.exists(rep["evaluation_info"]["checkpoint"])
