"""The two CLIs' DTW flags on the MI355X: ``evaluate_vanilla_gan_signatures --dtw [BAND]`` on a tiny randomly initialised
checkpoint the test writes, and ``signature_verifier_eval --dtw_baseline [BAND]`` on a small synthetic test directory.

The distances are integers, so the yardstick is exact: the numpy restatement (tests/dtwcommon.py) on the bytes the run itself
generated and on the files as the loaders decode them, reduced by the module's numpy reductions (dtw.dtw_diversity,
dtw.nearest_real_from_best) or, for the verifier baseline, by the evaluation's own roc_curve / auc on the negated distances.
Without the flags every report key and every printed line is what it was.

The Generator is reference_init's under a fixed seed with its final conv times 1024 (tests/test_ssim_cli_gpu.py): bytes on both
sides of 128."""
import glob
import json

import numpy as np
import pytest
import torch
from PIL import Image

import dtwcommon as DC
import verifiercommon as VC

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
    ck = tmp_path_factory.mktemp("dtw_cli") / "checkpoint.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": SIZE}}, ck)
    return ck


def real_images():
    family = DC.signature_family(SIZE, SIZE, 4, seed=2)
    return {"hand_a": family[0], "hand_b": family[1], "hand_c": family[2], "moved": DC.shifted(family[:1], 3)[0],
            "strokes": DC.stroke_image(SIZE, SIZE, 21), "noise": DC.sparse_noise(SIZE, SIZE, 9), "paper": np.full((SIZE, SIZE), 250, np.uint8)}


@pytest.fixture(scope="module")
def real_dir(tmp_path_factory):
    folder = tmp_path_factory.mktemp("dtw_real")
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


def as_json(d):
    return json.loads(json.dumps(d))


def test_evaluate_reports_the_restatements_reductions(checkpoint, real_dir, tmp_path, capsys):
    from signature_gan_amd import dtw
    from signature_gan_amd.utils import metrics
    plain = run_evaluate(checkpoint, tmp_path / "p", "--real_dir", str(real_dir))
    plain_text = capsys.readouterr().out
    assert "elastic_similarity" not in plain["metrics"] and "DTW" not in plain_text
    flagged = run_evaluate(checkpoint, tmp_path / "s", "--real_dir", str(real_dir), "--dtw")
    flagged_text = capsys.readouterr().out
    block = flagged["metrics"].pop("elastic_similarity")
    assert scrub(flagged) == scrub(plain)                                             # every other key of the report is what it was
    added = [line for line in flagged_text.splitlines() if "DTW" in line]
    assert len(added) == 3 and sum(line.startswith("DTW ") for line in added) == 2    # one progress line, two summary lines

    def comparable(text, out):
        return [line for line in text.replace(str(tmp_path / out), "OUT").splitlines() if "DTW" not in line and "evaluation_report_" not in line]
    assert comparable(flagged_text, "s") == comparable(plain_text, "p")               # and every other printed line

    fake, real = the_runs_bytes(checkpoint, real_dir)
    assert fake.shape == (N, SIZE, SIZE) and real.shape == (len(real_images()), SIZE, SIZE)
    assert len({im.tobytes() for im in fake}) == N                                    # the random Generator did not collapse
    band = DC.default_band(SIZE)
    pf, pr = DC.profiles(fake), DC.profiles(real)
    gg, rr, gr = DC.dtw_matrix(pf, pf, band), DC.dtw_matrix(pr, pr, band), DC.dtw_matrix(pf, pr, band)
    assert set(block) == {"band", "threshold", "diversity_images", "generated_diversity", "real_diversity", "nearest_real"}
    assert (block["band"], block["threshold"], block["diversity_images"]) == (band, 128, 512)
    assert block["generated_diversity"] == as_json(dtw.dtw_diversity(gg, SIZE)) and block["real_diversity"] == as_json(dtw.dtw_diversity(rr, SIZE))
    assert block["generated_diversity"]["all_pairs"]["pairs"] == N * (N - 1) // 2 > block["generated_diversity"]["lpips_pairs"]["pairs"] > 0
    assert block["generated_diversity"]["all_pairs"]["diversity"] > 0
    best, index = DC.first_minimum(gr)
    loo = DC.first_minimum(rr, skip_diagonal=True)[0]
    assert block["nearest_real"] == as_json(dtw.nearest_real_from_best(best, index, loo, SIZE))
    assert (block["nearest_real"]["n_generated"], block["nearest_real"]["n_real_loo"]) == (N, len(real))
    # the module's functions on the same bytes give the same numbers
    fake_dev, real_dev = torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda()
    assert as_json(metrics.calculate_dtw_diversity(fake_dev)) == block["generated_diversity"]
    assert as_json(metrics.calculate_dtw_nearest_real(fake_dev, real_dev)) == block["nearest_real"]
    assert metrics.calculate_dtw_diversity(fake_dev, max_images=4) == dtw.dtw_diversity(gg[:4, :4], SIZE)
    assert metrics.calculate_dtw_nearest_real(fake_dev, real_dev[:1])["real_loo_median"] is None
    # the moved copy of a real file and its original are each other's nearest: the shift is absorbed
    names = list(real_images())
    a, m = names.index("hand_a"), names.index("moved")
    real_best, real_index = dtw.dtw_best(real_dev)
    assert (real_index[a].item(), real_index[m].item()) == (m, a) and real_best[a].item() == rr[a, m]

    # an explicit band, and no real directory: only the generated diversity is reported
    alone = run_evaluate(checkpoint, tmp_path / "n", "--dtw", "2")["metrics"]["elastic_similarity"]
    assert set(alone) == {"band", "threshold", "diversity_images", "generated_diversity"} and alone["band"] == 2
    assert alone["generated_diversity"] == as_json(dtw.dtw_diversity(DC.dtw_matrix(pf, pf, 2), SIZE))


def write_test_dir(folder):
    """Three writers, three signatures each: one hand's variations per writer, as files of another size than the verifier's."""
    for u in range(3):
        (folder / f"user{u}").mkdir(parents=True)
        for k, img in enumerate(DC.signature_family(48, 96, 3, seed=40 + u)):
            Image.fromarray(img).save(str(folder / f"user{u}" / f"sig{k}.png"))


def test_the_verifier_evaluations_baseline_block(tmp_path, capsys):
    from signature_gan_amd import signature_verifier_eval as SV
    data = tmp_path / "test"
    write_test_dir(data)
    model = str(tmp_path / "augmented.pth")
    torch.save({"model_state_dict": VC.torch_state(128), "embedding_dim": 128, "val_accuracy": 0.875, "epoch": 3,
                "includes_synthetic": True}, model)
    base = ["--augmented_model", model, "--test_dir", str(data), "--batch_size", "4", "--pairs_per_user", "3", "--device", "cuda"]

    def run(out, *flags):
        SV.main(base + ["--output_dir", str(tmp_path / out), *flags])
        text = capsys.readouterr().out.replace(str(tmp_path / out), "OUT")
        report = json.load(open(tmp_path / out / "evaluation_report.json"))
        report.pop("evaluation_timestamp")
        return report, text.splitlines()

    plain, plain_lines = run("p")
    assert "dtw_baseline" not in plain and not any("DTW" in line for line in plain_lines)
    flagged, flagged_lines = run("d", "--dtw_baseline")
    block = flagged.pop("dtw_baseline")
    assert flagged == plain                                                           # not a model row: everything else is what it was
    added = [line for line in flagged_lines if "DTW" in line]
    assert len(added) == 1 and added[0].startswith("DTW BASELINE (no training, band 8)")
    assert [line for line in flagged_lines if "DTW" not in line] == plain_lines

    # the same pairs, scored by the restatement and reduced by the evaluation's own roc_curve / auc
    ds = SV.SignatureTestDataset(str(data), pairs_per_user=3)
    pairs = [ds.get_uint8(i) for i in range(len(ds))]
    first, second = np.stack([p[0].numpy() for p in pairs]), np.stack([p[1].numpy() for p in pairs])
    y = np.array([int(p[2]) for p in pairs])
    distance = np.diag(DC.dtw_matrix(DC.profiles(first), DC.profiles(second), 8))

    def scores(y, d):
        fpr, tpr, _ = SV.roc_curve(y, -d.astype(np.float64))
        eer, threshold = SV.compute_eer_from_scores(y, -d.astype(np.float64))
        return {"auc": SV.auc(fpr, tpr), "eer": eer, "eer_distance": -threshold}
    want = {"band": 8, "pairs": len(ds), "genuine": int((y == 1).sum()), "forgery": int((y == 0).sum()), **scores(y, distance)}
    print(f"the baseline's block on {len(ds)} pairs: {block}")
    assert block == want and block["pairs"] == 18 and block["genuine"] == block["forgery"] == 9
    assert block["auc"] > 0.5                                                         # one hand's variations are closer than two hands

    # with --all_pairs the block also covers every pair, from one matrix; an explicit band
    both, both_lines = run("a", "--all_pairs", "--dtw_baseline", "4")
    block = both["dtw_baseline"]
    _, paths, writer_of = SV.list_signatures(str(data))
    every = np.stack([SV.load_uint8(p) for p in paths])
    matrix = DC.dtw_matrix(DC.profiles(every), DC.profiles(every), 4)
    i, j = np.triu_indices(len(paths), 1)
    same = (writer_of[i] == writer_of[j]).astype(np.int64)
    assert block["band"] == 4 and block["all_pairs"] == {"pairs": 36, "genuine": 9, "forgery": 27, **scores(same, matrix[i, j])}
    assert {k: v for k, v in block.items() if k != "all_pairs"} == \
        {"band": 4, "pairs": len(ds), "genuine": 9, "forgery": 9, **scores(y, np.diag(DC.dtw_matrix(DC.profiles(first), DC.profiles(second), 4)))}
    assert sum("DTW" in line for line in both_lines) == 1 and "all 36 pairs" in [line for line in both_lines if "DTW" in line][0]
    assert both["models"]["Augmented"]["all_pairs"] is not None
