"""The two CLIs' SSIM flags on the MI355X, on a tiny randomly initialised checkpoint the test writes:
``evaluate_vanilla_gan_signatures --ssim`` and ``generate_signatures --project PATH --project_ssim``.

The yardstick of the report is the float64 restatement (tests/ssimcommon.py) on the bytes the run itself generated and on the
real files as the loader decodes them, reduced by the same numpy reductions (ssim.ssim_diversity, ssim.nearest_real_from_best).
Values are held to the bound of test_ssim_gpu.py -- 16 x the largest deviation of the plain-fp32 restatement from the float64
one, here over every pair the report scores -- and an index is exact where the float64 gap between a row's two highest values
exceeds twice that bound, which cannot be closed by two values that each move by the bound; the inputs are drawn so that every
row qualifies, and the test asserts it.

The Generator is reference_init's under a fixed seed with its final conv times 1024 (tests/test_components_cli_gpu.py): bytes
on both sides of 128.  The real files are as unlike each other as the families allow (strokes, their inverse, noise, a shifted
copy, nearly white, nearly black), so a generated image's similarities to them are far apart."""
import glob
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import ssimcommon as SC

pytestmark = pytest.mark.gpu

LATENT, N, BATCH, SEEDV, SIZE = 100, 12, 5, 11, 64


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=LATENT, output_size=SIZE).to("cuda").eval()
    d = Discriminator(input_size=SIZE).to("cuda").eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
    g._engine.params_changed()
    ck = tmp_path_factory.mktemp("ssim_cli") / "checkpoint.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": SIZE}}, ck)
    return ck


def real_images():
    s0, s1, s2 = SC.strokes(SIZE, SIZE, 21), SC.strokes(SIZE, SIZE, 22), SC.strokes(SIZE, SIZE, 23)
    rng = np.random.default_rng(5)
    nearly_white = (255 - rng.integers(0, 40, (SIZE, SIZE))).astype(np.uint8)
    nearly_black = rng.integers(0, 40, (SIZE, SIZE)).astype(np.uint8)
    return {"strokes_a": s0, "strokes_b": s1, "inverse": 255 - s2, "noise": SC.noise(SIZE, SIZE, 9), "shifted": SC.shifted(s0),
            "white": nearly_white, "black": nearly_black}


@pytest.fixture(scope="module")
def real_dir(tmp_path_factory):
    folder = tmp_path_factory.mktemp("ssim_real")
    for i, (name, img) in enumerate(real_images().items()):
        Image.fromarray(img, mode="L").save(folder / f"{i:02d}_{name}.png")
    return folder


class _Recorder:
    def __init__(self):
        self.batches = []

    def update(self, u8):
        self.batches.append(u8.cpu().numpy().copy())


def run_evaluate(checkpoint, out, *flags):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    assert ev.main(["--checkpoint", str(checkpoint), "--n_samples", str(N), "--batch_size", str(BATCH), "--seed", str(SEEDV),
                    "--n_grids", "0", "--output_dir", str(out), *flags]) == 0
    (path,) = glob.glob(str(out / "evaluation_report_*.json"))
    return json.load(open(path))


def the_runs_bytes(checkpoint, real_dir):
    """(generated (N, S, S), real (R, S, S)) uint8: the same seed, loading and batches as the run; the files as the loader decodes them."""
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd.data_loader_signatures import SignatureDataset
    torch.manual_seed(SEEDV); np.random.seed(SEEDV)
    generator, _ = ev.load_generator_from_checkpoint(checkpoint, torch.device("cuda"))
    rec = _Recorder()
    ev.generate_samples(generator, N, generator.latent_dim, torch.device("cuda"), BATCH, keep_images=0, component_sink=rec)
    ds = SignatureDataset(real_dir)
    return np.concatenate(rec.batches).reshape(N, SIZE, SIZE), np.stack([ds.decode(i, SIZE) for i in range(len(ds))])


def scrub(report):
    """A report without what differs between any two runs: time stamps and the output folder."""
    report = json.loads(json.dumps(report))
    report["metrics"].pop("metrics_computed_at")
    report["evaluation_info"].pop("evaluation_timestamp")
    return report


def test_evaluate_reports_the_restatements_reductions(checkpoint, real_dir, tmp_path):
    from signature_gan_amd import ssim
    plain = run_evaluate(checkpoint, tmp_path / "p1", "--real_dir", str(real_dir))
    plain2 = run_evaluate(checkpoint, tmp_path / "p2", "--real_dir", str(real_dir))
    assert "pixel_similarity" not in plain["metrics"] and scrub(plain) == scrub(plain2)
    flagged = run_evaluate(checkpoint, tmp_path / "s", "--real_dir", str(real_dir), "--ssim")
    block = flagged["metrics"].pop("pixel_similarity")
    assert scrub(flagged) == scrub(plain)                                             # every other byte of the report is what it was

    fake, real = the_runs_bytes(checkpoint, real_dir)
    assert fake.shape == (N, SIZE, SIZE) and real.shape == (len(real_images()), SIZE, SIZE)
    assert len({im.tobytes() for im in fake}) == N                                    # the random Generator did not collapse
    gg, rr, gr = SC.ssim_matrix64(fake, fake), SC.ssim_matrix64(real, real), SC.ssim_matrix64(fake, real)
    deviation = max(float(np.abs(SC.ssim_matrix32(a, b).astype(np.float64) - m).max())
                    for a, b, m in ((fake, fake, gg), (real, real, rr), (fake, real, gr)))
    bound = SC.MARGIN * deviation
    print(f"fp32 restatement deviates {deviation:.3e}, bound {bound:.3e}")
    assert 1e-7 < deviation < 1e-4

    assert block["window"] == {"taps": 11, "sigma": 1.5, "weights": [float(v) for v in SC.taps()], "dynamic_range": 255,
                               "valid_positions_only": True}
    for key, m in (("generated_diversity", gg), ("real_diversity", rr)):
        want, got = ssim.ssim_diversity(m), block[key]
        assert got["n"] == want["n"]
        for pairs in ("lpips_pairs", "all_pairs"):
            assert got[pairs]["pairs"] == want[pairs]["pairs"] > 0
            print(f"{key}.{pairs}: {got[pairs]['mean_ssim']:.6f}, restatement {want[pairs]['mean_ssim']:.6f}")
            assert abs(got[pairs]["mean_ssim"] - want[pairs]["mean_ssim"]) <= bound
            assert got[pairs]["diversity"] == 1.0 - got[pairs]["mean_ssim"]
    assert block["generated_diversity"]["all_pairs"]["pairs"] == N * (N - 1) // 2 > block["generated_diversity"]["lpips_pairs"]["pairs"]

    # nearest real: every row's two highest float64 values are further apart than two values moving by the bound can close
    def gap(m):
        top = np.sort(m, axis=1)
        return top[:, -1] - top[:, -2]
    loo = rr.copy()
    np.fill_diagonal(loo, -np.inf)
    print(f"smallest top-two gap: generated to real {gap(gr).min():.3e}, real leave-one-out {gap(loo).min():.3e}; "
          f"twice the bound {2 * bound:.3e}")
    assert (gap(gr) > 2 * bound).all() and (gap(loo) > 2 * bound).all()
    want = ssim.nearest_real_from_best(gr.max(axis=1), gr.argmax(axis=1), loo.max(axis=1))
    got = block["nearest_real"]
    assert (got["n_generated"], got["n_real_loo"]) == (N, len(real))
    for key in ("mean", "median", "max", "real_loo_median"):
        print(f"nearest_real.{key}: {got[key]:.6f}, restatement {want[key]:.6f}")
        assert abs(got[key] - want[key]) <= bound, key
    assert got["excess_median"] == got["median"] - got["real_loo_median"]             # of two values that each hold the bound
    # the device's own indices for every row, and the report's five closest
    fake_set, real_set = ssim.SsimSet(torch.from_numpy(fake).cuda()), ssim.SsimSet(torch.from_numpy(real).cuda())
    best, index = ssim.ssim_best(fake_set, real_set)
    assert np.array_equal(index.cpu().numpy(), gr.argmax(axis=1))
    assert np.array_equal(ssim.ssim_best(real_set)[1].cpu().numpy(), loo.argmax(axis=1))
    assert np.abs(best.cpu().numpy().astype(np.float64) - gr.max(axis=1)).max() <= bound
    assert [tuple(c) for c in got["closest"]] == ssim.nearest_real_from_best(best, index)["closest"] and len(got["closest"]) == 5
    for (gi, ri, v), (_, _, wv) in zip(got["closest"], want["closest"]):
        assert ri == int(gr[gi].argmax()) and abs(v - gr[gi].max()) <= bound and abs(v - wv) <= bound

    # without a real directory only the generated diversity is reported
    alone = run_evaluate(checkpoint, tmp_path / "n", "--ssim")["metrics"]["pixel_similarity"]
    assert set(alone) == {"window", "diversity_images", "generated_diversity"}
    assert alone["generated_diversity"] == block["generated_diversity"]


def test_the_metric_functions_take_bytes_and_fp32(checkpoint, real_dir):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import ssim
    from signature_gan_amd.utils import metrics
    generator, _ = ev.load_generator_from_checkpoint(checkpoint, torch.device("cuda"))
    torch.manual_seed(3)
    u8, _, f32 = generator._engine.g_generate_u8(torch.randn(6, LATENT, device="cuda"), threshold=0.5, want_f32=True)
    want = ssim.ssim_diversity(ssim.ssim_matrix(u8.reshape(6, SIZE, SIZE).contiguous()))
    assert metrics.calculate_ssim_diversity(u8) == want == metrics.calculate_ssim_diversity(f32) == metrics.calculate_ssim_diversity(f32.cpu())
    assert metrics.calculate_ssim_diversity(u8, max_images=4) == ssim.ssim_diversity(ssim.ssim_matrix(u8[:4].reshape(4, SIZE, SIZE).contiguous()))
    real = torch.from_numpy(np.stack(list(real_images().values()))).cuda()
    near = metrics.calculate_ssim_nearest_real(u8, real)
    best, index = ssim.ssim_best(u8.reshape(6, SIZE, SIZE).contiguous(), real)
    assert near == ssim.nearest_real_from_best(best, index, ssim.ssim_best(real)[0]) == metrics.calculate_ssim_nearest_real(f32, real.cpu())
    assert metrics.calculate_ssim_nearest_real(u8, real[:1])["real_loo_median"] is None


def test_project_ssim_is_ssim_paired_on_the_written_pngs(checkpoint, tmp_path):
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd import ssim
    from signature_gan_amd.utils.inference import load_target_images
    src = tmp_path / "targets"
    src.mkdir()
    for name, img in list(real_images().items())[:3]:
        Image.fromarray(img, mode="L").save(src / f"{name}.png")
    base = ["--checkpoint", str(checkpoint), "--seed", "3", "--prefix", "sig", "--project", str(src), "--project_steps", "4"]
    cli.main(base + ["--output_dir", str(tmp_path / "a")])
    cli.main(base + ["--output_dir", str(tmp_path / "b"), "--project_ssim"])
    before, after = json.load(open(tmp_path / "a" / "sig_projection.json")), json.load(open(tmp_path / "b" / "sig_projection.json"))
    assert all("ssim" not in r for r in before) and [{k: v for k, v in r.items() if k != "ssim"} for r in after] == before
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    files, targets = load_target_images(str(src), SIZE)
    assert [r["file"] for r in after] == files
    recon = np.stack([np.array(Image.open(tmp_path / "b" / r["reconstruction"]).convert("L")) for r in after])
    want = ssim.ssim_paired(torch.from_numpy(np.ascontiguousarray(targets)).cuda(), torch.from_numpy(recon).cuda()).cpu().numpy()
    assert [r["ssim"] for r in after] == [float(v) for v in want]
    m64 = SC.ssim_matrix64(np.asarray(targets), recon)                                 # the bound of test_ssim_gpu.py over these images
    bound = SC.MARGIN * float(np.abs(SC.ssim_matrix32(np.asarray(targets), recon).astype(np.float64) - m64).max())
    assert np.abs(want.astype(np.float64) - np.diag(m64)).max() <= bound
