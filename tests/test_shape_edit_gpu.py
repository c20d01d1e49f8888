"""Shape-attribute editing on the GPU: utils.inference.edit_latents and the two CLIs' flags on top of the shape calls.

The loop is the manual composition Engine.g_forward -> shape.shape_grad -> the seeded Engine.g_latent_objective_grad -> torch add
-> Engine.op_adam bit for bit (every dz is read off the loop's own op_adam calls).  The case: latentcommon's 64x64 Generator,
two of its start vectors, three steps.  Whether an edit reaches its target depends on the checkpoint and is printed, not
asserted."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from latentcommon import P_BETAS, P_LATENT, P_LR, P_SIZE, projection_case

pytestmark = pytest.mark.gpu
N, STEPS = 2, 3
EDIT = dict(slant_delta=-0.2, size_scale=1.1, boldness_scale=1.2, shift=(0.02, -0.01))
KEEP, SHAPE_W = 0.5, 2.0


@pytest.fixture(scope="module")
def case():
    from signature_gan_amd.generator_vanilla_gan import Generator
    sd, _, z0 = projection_case()
    g = Generator(latent_dim=P_LATENT, output_size=P_SIZE).to("cuda:0")
    g.load_state_dict(sd)
    g.eval()
    return dict(g=g, z0=z0[:N].clone(), sd=sd)


def full_objective(eng, z, keep_u8, w, t):
    """The manual composition at z: (dz, keep objective + shape objective, features)."""
    from signature_gan_amd import shape as S
    img = eng.g_forward(z, training=False)
    dx, shape_obj, feats = S.shape_grad(img, w, t)
    dz, obj = eng.g_latent_objective_grad(z, keep_u8, KEEP, 0.0, 0.0, image_grad=dx)
    return dz, obj + shape_obj, feats


def test_loop_is_the_manual_composition_bit_for_bit(case, monkeypatch):
    from signature_gan_amd import shape as S
    from signature_gan_amd.utils.inference import edit_latents, edit_targets, generate_uint8
    g = case["g"]
    eng = g._require_engine()
    state_before = {k: v.detach().clone() for k, v in g.state_dict().items()}
    # the manual chain
    z = case["z0"].clone().cuda()
    f0 = S.shape_features(eng.g_forward(z, training=False))
    w, t = edit_targets(f0, shape_weight=SHAPE_W, **EDIT)
    keep_u8 = torch.from_numpy(generate_uint8(g, z)).cuda()
    m, s = torch.zeros_like(z), torch.zeros_like(z)
    hist, dzs = [], []
    for k in range(STEPS):
        dz, obj, _ = full_objective(eng, z, keep_u8, w, t)
        hist.append(obj.clone()); dzs.append(dz.clone())
        eng.op_adam(z, dz, m, s, k + 1, lr=P_LR, beta1=P_BETAS[0], beta2=P_BETAS[1])
    _, final, f_final = full_objective(eng, z, keep_u8, w, t)
    # the loop, every dz read off its own op_adam calls
    seen = []
    orig = eng.op_adam
    monkeypatch.setattr(eng, "op_adam", lambda z_, dz_, *a, **kw: (seen.append(dz_.clone()), orig(z_, dz_, *a, **kw))[1])
    lz, images, before, after, targets, history = edit_latents(g, case["z0"], steps=STEPS, lr=P_LR, betas=P_BETAS, keep_weight=KEEP,
                                                               shape_weight=SHAPE_W, **EDIT)
    assert len(seen) == STEPS and history.shape == (STEPS + 1, N)
    for k in range(STEPS):
        assert torch.equal(seen[k], dzs[k]) and torch.equal(history[k], hist[k]), k
    assert torch.equal(lz, z) and torch.equal(history[STEPS], final)               # the objective AT the returned z
    assert torch.equal(before, f0) and torch.equal(targets, t) and torch.equal(after, f_final)
    assert np.array_equal(images, generate_uint8(g, z)) and images.shape == (N, P_SIZE, P_SIZE)
    # the shape term is there: dz is not the keep-only dz, and the objective is above the keep-only objective
    z_start = case["z0"].clone().cuda()
    dz_keep, obj_keep = eng.g_latent_objective_grad(z_start, keep_u8, KEEP, 0.0, 0.0)
    assert not torch.equal(dzs[0], dz_keep) and bool((hist[0] > obj_keep).all())
    # nothing of the Generator moved
    for k, v in g.state_dict().items():
        assert torch.equal(v, state_before[k]), k
    names = S.FEATURES
    for i in range(N):
        print(f"image {i} (an observation; {STEPS} steps): " + ", ".join(
            f"{names[k]} {float(before[i, k]):+.5f} -> {float(after[i, k]):+.5f} (target {float(targets[i, k]):+.5f})"
            for k in (S.MASS, S.CX, S.CY, S.SLANT, S.SPREAD)))
    print(f"objective: {history[0].tolist()} -> {history[STEPS].tolist()}")


def test_keep_weight_zero_runs_without_a_target_and_no_edit_raises(case):
    from signature_gan_amd.utils.inference import edit_latents
    g = case["g"]
    z, images, before, after, targets, history = edit_latents(g, case["z0"], slant_delta=0.1, steps=2, keep_weight=0.0)
    assert history.shape == (3, N) and bool(torch.isfinite(history).all()) and bool((history[0] > 0).all())
    assert not torch.equal(z.cpu(), case["z0"])
    with pytest.raises(ValueError, match="no edit"):
        edit_latents(g, case["z0"])
    with pytest.raises(ValueError, match="no edit"):
        edit_latents(g, case["z0"], slant_delta=0.0, size_scale=1.0, boldness_scale=1.0, shift=(0.0, 0.0))
    with pytest.raises(ValueError):
        edit_latents(g, case["z0"], slant_delta=0.1, realism_weight=1.0)           # no Discriminator
    g.train()
    try:
        with pytest.raises(ValueError, match="eval"):
            edit_latents(g, case["z0"], slant_delta=0.1)
    finally:
        g.eval()


def file_bytes(folder):
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


@pytest.fixture(scope="module")
def checkpoint(case, tmp_path_factory):
    ck = tmp_path_factory.mktemp("shape_cli") / "g.pt"
    torch.save({"epoch": 1, "generator_state_dict": case["sd"], "config": {"latent_dim": P_LATENT, "image_size": P_SIZE}}, ck)
    return ck


def test_generate_cli_edits_the_plain_runs_latents(case, checkpoint, tmp_path):
    from PIL import Image
    from signature_gan_amd import generate_signatures as cli
    from signature_gan_amd import shape as S
    from signature_gan_amd.utils.inference import edit_latents
    base = ["--checkpoint", str(checkpoint), "--n_samples", "5", "--batch_size", "3", "--seed", "3", "--prefix", "sig"]
    cli.main(base + ["--output_dir", str(tmp_path / "a")])
    cli.main(base + ["--output_dir", str(tmp_path / "b")])
    plain = file_bytes(tmp_path / "a")
    assert plain == file_bytes(tmp_path / "b") and sorted(plain) == [f"sig_{i + 1:06d}.png" for i in range(5)]   # no new file without the flag
    cli.main(base + ["--output_dir", str(tmp_path / "e"), "--edit", "--edit_slant_delta", "-0.2", "--edit_shift", "0.02", "0",
                     "--edit_steps", "2", "--edit_keep", "0.5"])
    assert sorted(os.listdir(tmp_path / "e")) == sorted(list(plain) + ["sig_edit.json"])
    report = json.load(open(tmp_path / "e" / "sig_edit.json"))
    assert report["edit"] == dict(slant_delta=-0.2, size_scale=1.0, boldness_scale=1.0, shift=[0.02, 0.0], steps=2, lr=0.02,
                                  keep_weight=0.5, realism_weight=0.0)
    rec = report["records"]
    assert [r["file"] for r in rec] == sorted(plain)
    # the same latents as the plain run: seeded once, then one draw per batch
    torch.manual_seed(3); torch.cuda.manual_seed_all(3)
    zs = [torch.randn(b, P_LATENT, device="cuda") for b in (3, 2)]
    want = [edit_latents(case["g"], z, slant_delta=-0.2, shift=(0.02, 0.0), steps=2, keep_weight=0.5) for z in zs]
    images = np.concatenate([w[1] for w in want])
    before, after, targets = (torch.cat([w[k] for w in want]).cpu().numpy() for k in (2, 3, 4))
    history = torch.cat([w[5] for w in want], dim=1).cpu().numpy()
    plain_features = S.features_from_sums(S.reference_sums_u8(np.stack([np.array(Image.open(tmp_path / "a" / n)) for n in sorted(plain)])), P_SIZE)
    for i, r in enumerate(rec):
        assert set(r) == {"file", "before", "targets", "after", "objective_before", "objective_after"}
        assert set(r["before"]) == set(r["after"]) == set(S.FEATURES) and set(r["targets"]) == {"cx", "cy", "slant"}
        assert [r["before"][n] for n in S.FEATURES] == before[i].tolist() and [r["after"][n] for n in S.FEATURES] == after[i].tolist()
        assert r["targets"]["slant"] == targets[i, S.SLANT] and r["targets"]["cx"] == targets[i, S.CX]
        assert r["objective_before"] == float(history[0, i]) and r["objective_after"] == float(history[-1, i])
        assert np.array_equal(np.array(Image.open(tmp_path / "e" / r["file"])), images[i])
        # "before" describes the plain run's image i: its fp32 features against the written bytes', to the quantisation
        assert abs(r["before"]["cx"] - plain_features[i, S.CX]) < 0.01 and abs(r["before"]["mass"] - plain_features[i, S.MASS]) < 0.01
    print("edit (synthetic state, an observation):", [(r["before"]["slant"], r["targets"]["slant"], r["after"]["slant"]) for r in rec])


def test_evaluate_cli_reports_shape_attributes(checkpoint, tmp_path):
    from PIL import Image
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    from signature_gan_amd import shape as S
    from signature_gan_amd.data_loader_signatures import SignatureDataset
    from signature_gan_amd.utils.metrics import calculate_shape_attributes, shape_attributes_from_features
    real_dir = tmp_path / "real"
    real_dir.mkdir()
    rng = np.random.default_rng(4)
    for i in range(5):
        Image.fromarray(rng.integers(0, 256, size=(P_SIZE, P_SIZE), dtype=np.uint8), mode="L").save(real_dir / f"{i:02d}.png")
    common = ["--checkpoint", str(checkpoint), "--n_samples", "11", "--batch_size", "4", "--seed", "5", "--n_grids", "0", "--real_dir", str(real_dir)]

    def run(out, *flags):
        assert ev.main(common + ["--output_dir", str(out), *flags]) == 0
        (path,) = glob.glob(str(out / "evaluation_report_*.json"))
        return json.load(open(path))

    plain = run(tmp_path / "p")
    assert "shape_attributes" not in plain["metrics"]
    with_flag = run(tmp_path / "s", "--shape")
    block = with_flag["metrics"].pop("shape_attributes")
    drop = lambda m: {k: v for k, v in m.items() if k != "metrics_computed_at"}      # noqa: E731
    assert drop(with_flag["metrics"]) == drop(plain["metrics"]) and with_flag["summary"] == plain["summary"]
    assert list(block) == ["generated", "real"]
    ds = SignatureDataset(real_dir)
    real = np.stack([ds.decode(i, P_SIZE) for i in range(len(ds))])
    want_real = shape_attributes_from_features(S.features_from_sums(S.reference_sums_u8(real), P_SIZE))
    assert block["real"] == want_real and want_real["images"] == 5
    assert block["real"] == calculate_shape_attributes(torch.from_numpy(real))
    g = block["generated"]
    assert g["images"] == 11 and set(g) == {"images", "empty", *S.FEATURES} and set(g["slant"]) == {"mean", "std", "p5", "p50", "p95"}
    # fp32 images go through the fp64 kernel: the same summary to the dequantisation of the bytes
    fp32 = torch.from_numpy(real.astype(np.float32) / 127.5 - 1.0).unsqueeze(1)
    soft = calculate_shape_attributes(fp32)
    assert abs(soft["cx"]["mean"] - want_real["cx"]["mean"]) < 1e-5 and soft["images"] == 5
