"""The ablation study's LeakyReLU Generator (siggan_config.g_leaky_slope, Engine(g_activation='leaky_relu'),
signature_gan_amd.ablation_vanilla_gan_signatures) on the MI355X.

Chain of the fp32 parity tests (test_engine_gpu.test_ablation_step_variant): the HIP path against the oracle's restatement
(oracle.siggan_oracle with g_slope / slope = common.SLOPE) given the HIP path's own activation-sign decisions (arithmetic,
1e-4 of scale), the restatement given the reference run's decisions (fixture census) against the fixture, and the HIP
decisions that differ from the reference's counted against the census."""
import os

import numpy as np
import pytest
import torch

from common import (GOLDEN, SLOPE, I, O, SEED, ablation_groups, assert_close, census_signs, d_chans, flips_vs_census, oracle_states,
                    oracle_states_sn, probe)

pytestmark = pytest.mark.gpu

from test_ablation_leaky_cpu import LEAKY_CASES      # noqa: E402  (size, latent, batch, spectral norm)


def _fixture():
    return np.load(os.path.join(GOLDEN, "golden_ablation_leaky.npz"))


def _engine(size, latent, batch, warm=True, dtype="f32", spectral_norm=False, seed=0):
    from hipcommon import load_engine_state
    from signature_gan_amd.engine import Engine
    eng = Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", seed=seed, dtype=dtype,
                 spectral_norm=spectral_norm, g_activation="leaky_relu", g_leaky_slope=SLOPE)
    return load_engine_state(eng, size, latent, warm)


def _scale(grads, names):
    top = max(float(grads[k].abs().max()) for k in names)
    return {k: max(float(grads[k].abs().max()), 1e-3 * top) for k in names}


def _worst(got, want, scale):
    return max(float((got[k].cpu() - want[k]).abs().max()) / scale[k] for k in want)


def _golden_worst(f, tag, grads, scale):
    return max(float(np.abs(probe(grads[k].cpu(), k) - f[f"{tag}/grad/{k}"]).max()) / scale[k] for k in scale)


@pytest.mark.parametrize("size,latent,batch,sn", LEAKY_CASES)
def test_leaky_ablation_iteration_vs_restatement_and_reference(size, latent, batch, sn):
    """Each fixture case; (64, 50, 8) runs the Generator fc's generic kernels (latent % 4 != 0: k_fc_fwd, k_bn_relu,
    k_colreduce<FBnBwd> + k_bn_bwd_apply) against a spectral-norm Discriminator (a power iteration in each of the three
    train-mode D passes)."""
    from hipcommon import count_sign_flips, cuda, hip_ablation_iteration
    f = _fixture()
    tag = f"s{size}_z{latent}_b{batch}" + ("_sn" if sn else "")
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, d_chans(size) * 3)]
    nb = len(masks) // 3
    z = torch.from_numpy(f[f"{tag}/z"])
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    eng = _engine(size, latent, batch, spectral_norm=sn)
    if sn:
        for k, v in eng.sn_views().items():
            v.copy_(oracle_states_sn(size, latent)[4][k])
    eng.set_step_variant("ablation")
    met, hip, keep, d_hip, g_hip, p_hip = hip_ablation_iteration(eng, real, z, masks, size, batch)

    def run(signs, rec, preds=None):
        g_sd, d_sd, g_opt, d_opt, sn_uv = oracle_states_sn(size, latent, sn)
        o = O.ablation_step(g_sd, d_sd, g_opt, d_opt, real, z, masks[:nb], masks[nb:2 * nb], masks[2 * nb:], size,
                            signs=signs, record=rec, g_slope=SLOPE, sn=sn_uv, preds=preds)
        return o, sn_uv
    rec, o_preds = {}, []
    (o_met, o_dg, o_gg), o_sn = run(hip, rec, o_preds)
    # per-sample D predictions of the three passes: vs the restatement (arithmetic) and vs the reference
    assert float((p_hip - torch.stack(o_preds)).abs().max()) <= 2e-4, "D predictions vs restatement"
    assert float(np.abs(p_hip.numpy() - f[f"{tag}/preds"]).max()) <= 1e-3, "D predictions vs reference"
    if sn:                                                   # three power iterations later
        for k, v in eng.sn_views().items():
            v = v.cpu()
            assert float((v - o_sn[k]).abs().max()) <= 1e-4 * float(o_sn[k].abs().max()), f"{k} vs restatement"
            want = f[f"{tag}/d/sn/{k}"]
            assert float(np.abs(probe(v, k) - want).max()) <= 1e-3 * float(np.abs(want).max()), f"{k} vs reference"
    for grp in hip:
        count_sign_flips(hip[grp], rec[grp], keep=keep[grp])
    for k, v in o_met.items():
        assert_close(met[k], v, 2e-4, 2e-6, f"leaky ablation metric {k} vs restatement")
        key = f"{tag}/{k[0]}/metric/{k}"
        if key in f:
            assert_close(met[k], f[key], 1e-3, 1e-5, f"leaky ablation metric {k} vs reference")
    sc_d, sc_g = _scale(o_dg, list(o_dg)), _scale(o_gg, list(o_gg))
    assert _worst(d_hip, o_dg, sc_d) <= 2e-4 and _worst(g_hip, o_gg, sc_g) <= 1e-4      # the bars of test_ablation_step_variant
    # the reference's own decisions -> the fixture
    (c_met, c_dg, c_gg), _ = run(ablation_groups(size, census_signs(f, tag)), None)
    assert max(_golden_worst(f, f"{tag}/d", c_dg, sc_d), _golden_worst(f, f"{tag}/g", c_gg, sc_g)) <= 1e-4
    order = hip["d_real"] + hip["g"] + hip["d_fake"] + hip["d_g"]
    flips = flips_vs_census(f, tag, order, keep=list(masks[:nb]) + [None] * len(hip["g"]) + list(masks[nb:]))
    hip_vs_ref = max(_golden_worst(f, f"{tag}/d", d_hip, sc_d), _golden_worst(f, f"{tag}/g", g_hip, sc_g))
    if not flips:
        assert hip_vs_ref <= 1e-3, hip_vs_ref
    else:
        pred = max(_golden_worst(f, f"{tag}/d", o_dg, sc_d), _golden_worst(f, f"{tag}/g", o_gg, sc_g))
        assert abs(hip_vs_ref - pred) <= 1e-3, (hip_vs_ref, pred, len(flips))
    for k, t in eng.bn_views().items():
        want = f[f"{tag}/g/buf/{k}"]
        assert_close(probe(t.float().cpu(), k), want, 1e-3, 1e-3 * max(float(np.abs(want).max()), 1e-30), f"BN buffer {k}")
    # generate_samples after the iteration: eval mode (running statistics, BatchNorm folded into the epilogues).  Against the
    # restatement on the engine's own updated state: arithmetic, 1e-4.  Against the reference: the biases in front of a
    # train-mode BatchNorm have a gradient of pure rounding noise, which Adam turns into +-lr moves that BatchNorm cancels in
    # training but the eval forward sees (measured 1.8e-3 absolute at 128x128); the bound is 5e-3 of the image scale.
    from hipcommon import oracle_state_of
    ez = torch.from_numpy(f[f"{tag}/eval/z"])
    img = eng.g_forward(cuda(ez), training=False).cpu()
    with torch.no_grad():
        oimg = O.g_forward(oracle_state_of(eng, size, latent)[0], ez, False, size, slope=SLOPE)
    assert float((img - oimg).abs().max()) <= 1e-4 * float(oimg.abs().max()), "eval image vs restatement"
    want = f[f"{tag}/eval/img"]
    assert float(np.abs(img.numpy() - want).max()) <= 5e-3 * float(np.abs(want).max()), "eval image vs reference"
    eng.close()


def test_leaky_epoch_means_vs_reference():
    """Three Engine.ablation_step iterations driven with the fixture's z and masks: the reference's four epoch means."""
    from hipcommon import cuda
    f = _fixture()
    size, latent, batch, n = (int(v) for v in f["epoch/case"])
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f["epoch/masks"], batch, d_chans(size) * 3 * n)]
    per = len(masks) // n
    eng = _engine(size, latent, batch)
    eng.set_step_variant("ablation")
    sums = np.zeros(4)
    for k in range(n):
        real = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + k)))
        m = eng.ablation_step(real, cuda(torch.from_numpy(f["epoch/z"][k])), masks[k * per:(k + 1) * per])
        sums += [m["g_loss"], m["d_loss"], m["d_real_mean"], m["d_fake_mean"]]
    assert_close(sums / n, f["epoch/means"], 1e-3, 1e-5, "leaky epoch means vs reference")
    eng.close()


def test_leaky_trainer_variant_vs_restatement():
    """The trainer variant (GANTrainer's D step then G step) with a LeakyReLU Generator, 64x64, batch 16.  The reference never
    trains this combination (its trainer builds the ReLU Generator), so only the restatement pins it: HIP vs restatement given
    the HIP path's sign decisions, 1e-4 of scale."""
    from hipcommon import count_sign_flips, cuda, hip_signs_d, hip_signs_g
    size, latent, batch = 64, 100, 16
    z1 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, d_chans(size) * 2, 5)]
    nb = len(masks) // 2
    eng = _engine(size, latent, batch)
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
    dm = eng.d_step(cuda(real), cuda(z1), masks)
    signs, rec = hip_signs_d(eng, size, batch, 2), []
    odm, odg = O.d_step(g_sd, d_sd, d_opt, real, z1, masks[:nb], masks[nb:], size, signs=signs, record=rec, g_slope=SLOPE)
    count_sign_flips(signs, rec, keep=masks)
    dv = eng.views("d", "grads")
    assert _worst(dv, odg, _scale(odg, list(odg))) <= 1e-4
    for k in ("d_loss", "d_real_mean", "d_fake_mean"):
        assert_close(dm[k], odm[k], 2e-4, 2e-6, k)
    gm = eng.g_step(batch, cuda(z2))
    signs, rec = hip_signs_g(eng, size, batch) + hip_signs_d(eng, size, batch, 1), []
    ogm, ogg = O.g_step(g_sd, d_sd, g_opt, z2, size, signs=signs, record=rec, g_slope=SLOPE)
    count_sign_flips(signs, rec)
    assert _worst(eng.views("g", "grads"), ogg, _scale(ogg, list(ogg))) <= 1e-4
    for k in ("g_loss", "g_fake_mean"):
        assert_close(gm[k], ogm[k], 2e-4, 2e-6, k)
    img = eng.g_forward(cuda(z1), training=False).cpu()
    with torch.no_grad():
        oimg = O.g_forward(g_sd, z1, False, size, slope=SLOPE)
    assert float((img - oimg).abs().max()) <= 1e-4 * float(oimg.abs().max())
    eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_leaky_narrow_vs_fp32_restatement(dtype):
    """16-bit storage with the LeakyReLU Generator, free-running against the fp32 restatement at test_narrow_gpu's bars (1)."""
    from hipcommon import cuda
    from test_narrow_gpu import TOL_FP32
    tol = TOL_FP32[dtype]
    size, latent, batch = 64, 100, 16
    z1 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, d_chans(size) * 2, 5)]
    nb = len(masks) // 2
    eng = _engine(size, latent, batch, dtype=dtype)
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
    img = eng.g_forward(cuda(z1), training=False).cpu()
    with torch.no_grad():
        oimg = O.g_forward({k: v.clone() for k, v in g_sd.items()}, z1, False, size, slope=SLOPE)
    assert float((img - oimg).abs().max()) <= tol["image"]
    dm = eng.d_step(cuda(real), cuda(z1), masks)
    odm, odg = O.d_step(g_sd, d_sd, d_opt, real, z1, masks[:nb], masks[nb:], size, g_slope=SLOPE)
    gm = eng.g_step(batch, cuda(z2))
    ogm, ogg = O.g_step(g_sd, d_sd, g_opt, z2, size, g_slope=SLOPE)
    for got, want, keys in ((dm, odm, ("d_loss", "d_real_mean", "d_fake_mean")), (gm, ogm, ("g_loss", "g_fake_mean"))):
        for k in keys:
            assert abs(got[k] - want[k]) <= tol["metric"] * max(abs(want[k]), 1e-3), (dtype, k, got[k], want[k])
    hip = torch.cat([t.reshape(-1).cpu() for t in eng.views("g", "grads").values()])
    ref = torch.cat([ogg[k].reshape(-1) for k in eng.views("g", "grads")])
    assert float((hip - ref).norm() / ref.norm()) <= tol["grad_all"], dtype
    assert all(np.isfinite(v) for v in list(dm.values()) + list(gm.values()) if v is not None)
    eng.close()


def test_leaky_execution_modes_and_staging_are_bitwise_identical():
    """graph replay == overlap, and train_step with a staged next batch == d_step + g_step, bit for bit, with LeakyReLU."""
    from hipcommon import cuda
    size, latent, batch = 64, 100, 16
    real = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"])))
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, d_chans(size) * 2, 3)]

    def state(eng):
        return [t.clone() for t in (eng.g_params, eng.d_params, eng.g_exp_avg_sq, eng.d_exp_avg, eng.g_bn_mean, eng.g_bn_var)]

    runs = []
    for graph, overlap in ((True, False), (False, True)):
        eng = _engine(size, latent, batch)
        eng.set_mode(graph=graph, overlap=overlap)
        mets = []
        for s in range(3):
            mets.append(eng.d_step(real, cuda(torch.from_numpy(I.gen_z(batch, latent, 50 + s))), masks, clip=0.5))
            mets.append(eng.g_step(batch, cuda(torch.from_numpy(I.gen_z(batch, latent, 60 + s))), clip=0.5))
        runs.append((state(eng), mets))
        eng.close()
    assert runs[0][1] == runs[1][1]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b), "graph replay and overlap differ with the LeakyReLU Generator"

    reals = [cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + 7 * t))) for t in range(4)]
    zs = [(cuda(torch.from_numpy(I.gen_z(batch, latent, 70 + t))), cuda(torch.from_numpy(I.gen_z(batch, latent, 80 + t))))
          for t in range(3)]

    def run(staged):
        eng = _engine(size, latent, batch)
        mets = []
        for t in range(3):
            if staged:
                mets.append(eng.train_step(reals[t], zs[t][0], masks, zs[t][1], clip=0.5, next_real=reals[t + 1]))
            else:
                m = eng.d_step(reals[t], zs[t][0], masks, clip=0.5)
                m.update(eng.g_step(batch, zs[t][1], clip=0.5))
                mets.append(m)
        out = state(eng), mets
        eng.close()
        return out
    (sa, ma), (sb, mb) = run(False), run(True)
    for x, y in zip(ma, mb):
        assert {k: x[k] for k in set(x) & set(y)} == {k: y[k] for k in set(x) & set(y)}
    for a, b in zip(sa, sb):
        assert torch.equal(a, b), "train_step with a staged batch differs from d_step + g_step"


def test_ablation_trainer_epoch_equals_engine_ablation_steps(tmp_path):
    """AblationGANTrainer.train_epoch over three batches == Engine.ablation_step driven directly from the same RNG position."""
    from signature_gan_amd.ablation_vanilla_gan_signatures import AblationConfig, AblationGANTrainer
    size, latent, batch = 64, 50, 8
    batches = [torch.from_numpy(I.gen_real(batch, size, SEED["real"] + k)) for k in range(3)]
    cfg = AblationConfig(name="t", latent_dim=latent, activation="leaky_relu", image_size=size, batch_size=batch, epochs=1)
    torch.manual_seed(5)
    tr = AblationGANTrainer(cfg, [(b, 0) for b in batches], "cuda:0", tmp_path)
    assert tr.engine.g_slope == pytest.approx(0.2) and tr.engine.step_variant == "ablation"
    assert list(tr.generator.state_dict()) == list(O.g_state_specs(latent, size))
    load = lambda eng: __import__("hipcommon").load_engine_state(eng, size, latent, True)
    load(tr.engine)
    tr.engine.seed(99)
    means = tr.train_epoch()
    assert tr.g_losses == [means[0]] and tr.d_losses == [means[1]] and len(tr.d_real_scores) == len(tr.d_fake_scores) == 1
    eng = _engine(size, latent, batch)
    eng.set_step_variant("ablation")
    eng.seed(99)
    ms = [eng.ablation_step(b.to("cuda:0")) for b in batches]
    want = tuple(sum(m[k] for m in ms) / 3 for k in ("g_loss", "d_loss", "d_real_mean", "d_fake_mean"))
    assert means == want
    assert torch.equal(tr.engine.g_params, eng.g_params) and torch.equal(tr.engine.d_params, eng.d_params)
    s = tr.generate_samples(5)
    assert s.shape == (5, 1, size, size) and not tr.generator.training and bool(torch.isfinite(s).all())
    eng.close()


def test_leaky_spectral_norm_128_ablation_iteration_runs():
    from hipcommon import cuda
    size, latent, batch = 128, 128, 4
    eng = _engine(size, latent, batch, spectral_norm=True)
    eng.set_step_variant("ablation")
    m = eng.ablation_step(cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"]))))
    assert all(np.isfinite(v) for v in m.values() if v is not None)
    assert bool(torch.isfinite(eng.g_params).all()) and bool(torch.isfinite(eng.d_params).all())
    img = eng.g_forward(torch.randn(batch, latent, device="cuda:0"), training=False)
    assert bool(torch.isfinite(img).all())
    eng.close()


def test_engine_refuses_a_bad_generator_slope():
    from signature_gan_amd.engine import Engine
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="g_leaky_slope"):
            Engine(latent_dim=100, image_size=64, max_batch=4, device="cuda:0", g_activation="leaky_relu", g_leaky_slope=bad)


def test_leaky_eval_forward_at_batch_64_vs_restatement():
    """An eval-mode Generator forward at 64x64, batch 64 (what AblationGANTrainer._save_samples runs on its 64 fixed_noise
    rows): the last block's fp32 GEMM takes the four-parity-class kernel (k_gconv_up4) there, whose LeakyReLU epilogue the
    smaller batches of the tests above do not reach.  Against the restatement on the engine's state, 1e-4 of scale."""
    from hipcommon import cuda, oracle_state_of
    size, latent, batch = 64, 100, 64
    eng = _engine(size, latent, batch)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 5))
    eng.prof_enable(True)
    img = eng.g_forward(cuda(z), training=False).cpu()
    launched = {r["name"]: r["launches"] for r in eng.prof_read()}
    eng.prof_enable(False)
    assert launched.get("k_gconv_up4", 0) >= 1, launched
    with torch.no_grad():
        oimg = O.g_forward(oracle_state_of(eng, size, latent)[0], z, False, size, slope=SLOPE)
    assert float((img - oimg).abs().max()) <= 1e-4 * float(oimg.abs().max())
    eng.close()
