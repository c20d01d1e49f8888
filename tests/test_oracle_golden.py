"""Pin the oracle (oracle/siggan_oracle.py) against the reference's own outputs (golden fixtures).

CPU only.  Tolerances: fp32, rtol 1e-4 / small atol -- the oracle and the reference run the same
torch CPU kernels, so they normally agree to ~1e-6; Adam second-moment probes are tiny numbers
(1e-6 scale) and use a relative test."""
import numpy as np
import pytest
import torch

from common import (CASES, DK, GK, I, O, SEED, ablation_groups, assert_close, census_signs, flips_vs_census, load_golden, masks_from,
                    oracle_states, oracle_states_sn, probe)

RT, AT = 1e-4, 1e-6
SEQ3_RT, SEQ3_AT = 1e-4, 1e-5     # chained metrics of the three-step sequence (losses / mean predictions, O(0.1 .. 1))
FIXTURE_THREADS = 8               # torch CPU threads of the reference run that made the fixtures (their meta 'threads')


@pytest.fixture(autouse=True)
def _fixture_thread_count():
    """torch's CPU kernels split their work (and so their fp32 summation order) by the thread count: the oracle runs with
    the count the fixtures were made with, whatever count the host would give it."""
    n = torch.get_num_threads()
    torch.set_num_threads(FIXTURE_THREADS)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("size,latent,batch", CASES)
def test_forward_passes(size, latent, batch):
    f, meta = load_golden(size, batch, latent)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, _, _ = oracle_states(size, latent, warm=False)

    img = O.g_forward(g_sd, z, False, size)
    if "g_eval/img" in f:
        assert_close(img.numpy(), f["g_eval/img"], RT, AT, "g_eval image")
    flat = img.reshape(-1).numpy()
    assert_close(flat[I.probe_idx(flat.size, "img", 256)], f["g_eval/probe"], RT, AT, "g_eval probe")

    img = O.g_forward(g_sd, z, True, size)
    flat = img.reshape(-1).numpy()
    assert_close(flat[I.probe_idx(flat.size, "img", 256)], f["g_train/probe"], RT, AT, "g_train probe")
    for k in g_sd:
        if "running" in k or "num_batches" in k:
            assert_close(probe(g_sd[k].float(), k), f["g_train/buf/" + k], RT, AT, k)

    g_sd, d_sd, _, _ = oracle_states(size, latent, warm=False)
    assert_close(O.d_forward(d_sd, real, size).reshape(-1).numpy(), f["d_eval/probs"], RT, AT, "d_eval probs")
    feat = O.d_features(d_sd, real, size).reshape(-1).numpy()
    assert_close(feat[I.probe_idx(feat.size, "feat", 256)], f["d_eval/feat_probe"], RT, AT, "d features")
    masks = masks_from(f, "d_train/masks", batch, size, 1)
    assert_close(O.d_forward(d_sd, real, size, masks).reshape(-1).numpy(), f["d_train/probs"], RT, AT,
                 "d_train probs")


def _check_step(f, tag, names, metrics, grads, sd, opt, bufs=None):
    """The oracle was given the reference run's own near-zero sign decisions (fixture census), so what is compared is
    arithmetic only: 1e-4 on every gradient norm and, relative to the tensor's scale, on every gradient / moment probe."""
    for k, v in metrics.items():
        key = f"{tag}/metric/{k}"
        if v is not None and key in f:
            assert_close(v, f[key], 1e-4, 1e-6, key)
    gn = np.array([float(grads[k].norm()) for k in names])
    ref_gn = f[f"{tag}/grad_norm"]
    gscale = float(max(np.abs(f[f"{tag}/grad/{k}"]).max() for k in names))     # network-wide grad scale
    assert_close(gn, ref_gn, 1e-4, 1e-5 * float(ref_gn.max()), tag + " grad norms")
    for k, rn in zip(names, ref_gn):
        # a parameter whose gradient is mathematically zero (a bias in front of a train-mode
        # BatchNorm) carries rounding noise only: Adam turns that noise into +-lr-sized moves,
        # so its moments / weights are checked against that bound, not bit-for-bit.
        noise = rn < 1e-5 * float(ref_gn.max())
        tscale = max(float(np.abs(f[f"{tag}/grad/{k}"]).max()), 1e-3 * gscale)
        assert_close(probe(grads[k], k), f[f"{tag}/grad/{k}"], 0, 1e-4 * tscale, f"{tag} grad {k}")
        assert_close(probe(opt.m[k], k), f[f"{tag}/m/{k}"], 1e-3, 1e-4 * gscale, f"{tag} exp_avg {k}")
        assert_close(probe(opt.v[k], k), f[f"{tag}/v/{k}"], 1e-3, 1e-7 * gscale * gscale, f"{tag} exp_avg_sq {k}")
        assert_close(probe(sd[k], k), f[f"{tag}/w/{k}"], 1e-4, 2.5e-4 if noise else 2e-6, f"{tag} weight {k}")
    assert float(f[f"{tag}/adam_step"]) == opt.step
    if bufs:
        for k in bufs:
            assert_close(probe(sd[k].float(), k), f[f"{tag}/buf/{k}"], 1e-4, 1e-6, f"{tag} buffer {k}")


@pytest.mark.parametrize("size,latent,batch", CASES)
@pytest.mark.parametrize("tag", ["warm", "fresh", "clip"])
def test_single_steps(size, latent, batch, tag):
    f, meta = load_golden(size, batch, latent)
    clip = meta["clip"] if tag == "clip" else None
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))

    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=(tag != "fresh"))
    masks = masks_from(f, f"dstep_{tag}/masks", batch, size, 2)
    nb = len(masks) // 2
    met, grads = O.d_step(g_sd, d_sd, d_opt, real, z, masks[:nb], masks[nb:], size, clip=clip, signs=census_signs(f, "dstep"))
    if clip is not None:
        assert met["d_grad_norm"] > clip, "fixture was meant to have clipping active"
    _check_step(f, f"dstep_{tag}", d_opt.names, met, grads, d_sd, d_opt)

    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=(tag != "fresh"))
    met, grads = O.g_step(g_sd, d_sd, g_opt, z2, size, clip=clip, signs=census_signs(f, "gstep"))
    if clip is not None:
        assert met["g_grad_norm"] > clip
    bufs = [k for k in g_sd if k not in g_opt.names]
    _check_step(f, f"gstep_{tag}", g_opt.names, met, grads, g_sd, g_opt, bufs)


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 64), (128, 128, 32)])
def test_census_makes_the_oracle_host_independent(size, latent, batch):
    """A different host / thread count changes torch's fp32 summation order, so the free-running oracle lands a handful of
    near-zero activation inputs on the other side than the reference run did (16.7 M such inputs in the last Generator block
    at 128x128 batch 32; |x| ~ 1e-8 of the layer scale) and its gradients move by 1e-4..1e-3: that is the reference's noise
    against ITSELF.  Given the fixture's census the oracle must reproduce the fixture at 1e-4 whatever the thread count --
    which is what lets the GPU box's CPU (another host) anchor the HIP path to the reference run."""
    f, _ = load_golden(size, batch, latent)
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    ref = f["gstep_warm/grad_norm"]
    big = ref > 1e-5 * ref.max()
    prev = torch.get_num_threads()
    try:
        torch.set_num_threads(3)
        g_sd, d_sd, g_opt, _ = oracle_states(size, latent, warm=True)
        rec = []
        _, grads, _, _ = O.g_grads(dict(g_sd), d_sd, z2, size, signs=census_signs(f, "gstep"), record=rec)
    finally:
        torch.set_num_threads(prev)
    gn = np.array([float(grads[k].norm()) for k in g_opt.names])
    assert float((np.abs(gn - ref)[big] / ref[big]).max()) <= 1e-4
    # every decision this run would have taken differently is in the census (nothing away from zero differs)
    for l, i, v in flips_vs_census(f, "gstep", [x > 0 for x in rec]):
        assert abs(v) <= 1e-5, (l, i, v)


@pytest.mark.parametrize("size,latent,batch", CASES)
def test_three_step_sequence(size, latent, batch):
    """VanillaGAN.train_step three times over (vanilla_gan_model.py:308-336).  Every half-step of the fixture carries the
    reference run's near-zero activation census (seq3/d<s>, seq3/g<s>): given those decisions the oracle must reproduce the
    chained metrics like the single steps -- the free-running oracle needed 1e-3 here and only held it at 64x64."""
    f, meta = load_golden(size, batch, latent)
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
    masks = masks_from(f, "seq3/masks", batch, size, 6)
    nb = len(masks) // 6
    rows = []
    for s in range(3):
        zs = torch.from_numpy(I.gen_z(batch, latent, 1000 + 2 * s))
        zg = torch.from_numpy(I.gen_z(batch, latent, 1001 + 2 * s))
        ms = masks[2 * nb * s: 2 * nb * (s + 1)]
        dm, _ = O.d_step(g_sd, d_sd, d_opt, real, zs, ms[:nb], ms[nb:], size, signs=census_signs(f, f"seq3/d{s}"))
        gm, _ = O.g_step(g_sd, d_sd, g_opt, zg, size, signs=census_signs(f, f"seq3/g{s}"))
        rows.append([dm["d_loss"], dm["d_loss_real"], dm["d_loss_fake"], dm["d_real_mean"],
                     dm["d_fake_mean"], gm["g_loss"], gm["g_fake_mean"]])
    assert_close(np.array(rows), f["seq3/metrics"], SEQ3_RT, SEQ3_AT, "3-step metrics, oracle(reference's decisions) vs the reference")


def test_param_counts_match_reference_manifest():
    import json, os
    from common import GOLDEN
    man = json.load(open(os.path.join(GOLDEN, "checkpoint_manifest.json")))
    for size, latent in ((64, 100), (128, 128)):
        gs, ds = O.g_state_specs(latent, size), O.d_state_specs(size)
        n = lambda specs: sum(int(np.prod(s)) for s, kind in specs.values() if kind == "param")
        assert n(gs) == man[f"s{size}"]["g_params"] and n(ds) == man[f"s{size}"]["d_params"]
        ref_g = man[f"s{size}"]["layout_A"]["generator_state_dict"]
        assert list(ref_g) == list(gs)
        for k, (shape, _) in gs.items():
            assert ref_g[k]["tensor"] == list(shape), k
        ref_d = man[f"s{size}"]["layout_A"]["discriminator_state_dict"]
        assert list(ref_d) == list(ds)
        for k, (shape, _) in ds.items():
            assert ref_d[k]["tensor"] == list(shape), k


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 8), (128, 128, 4)])
def test_ablation_step(size, latent, batch):
    """The oracle's restatement of AblationGANTrainer.train_epoch's iteration (ablation_vanilla_gan_signatures.py:397-467)
    against the fixture replayed on the reference's own modules (tests/golden/make_golden.py::make_ablation_step)."""
    import os
    from common import GOLDEN, d_chans
    f = np.load(os.path.join(GOLDEN, "golden_ablation_step.npz"))
    tag = f"s{size}_b{batch}"
    chans = d_chans(size) * 3
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, chans)]
    nb = len(masks) // 3
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
    met, d_grads, g_grads = O.ablation_step(g_sd, d_sd, g_opt, d_opt, real, z, masks[:nb], masks[nb:2 * nb], masks[2 * nb:], size,
                                            signs=ablation_groups(size, census_signs(f, tag)))
    _check_step(f, f"{tag}/d", d_opt.names, {k: v for k, v in met.items() if k.startswith("d_")}, d_grads, d_sd, d_opt)
    bufs = [k for k in g_sd if k not in g_opt.names]
    _check_step(f, f"{tag}/g", g_opt.names, {k: v for k, v in met.items() if k.startswith("g_")}, g_grads, g_sd, g_opt, bufs)


def _sn_check(f, tag, names_plain, keys, met, grads, sd, opt, sn=None):
    """_check_step against a fixture whose parameter names carry weight_orig (and whose parameter ORDER is the SN module's:
    bias before weight_orig) -- compared by name.  The oracle is given the reference run's near-zero sign decisions (census),
    the chained G step included, so both steps are held to 1e-4 of the network's gradient scale."""
    ren = lambda k: k.replace(".weight", ".weight_orig") if (k.endswith(".weight") and f"{tag}/grad/{k}_orig" in f) else k
    for k in keys:
        assert_close(met[k], f[f"{tag}/metric/{k}"], 1e-4, 1e-6, f"{tag} metric {k}")
    gscale = max(float(g.abs().max()) for g in grads.values())
    ga = 1e-4 * gscale + 1e-9
    for k in names_plain:
        rk = ren(k)
        assert_close(probe(grads[k], rk), f[f"{tag}/grad/{rk}"], 1e-3, ga, f"{tag} grad {k}")
        assert_close(probe(opt.m[k], rk), f[f"{tag}/m/{rk}"], 1e-3, ga, f"{tag} exp_avg {k}")
        assert_close(probe(sd[k], rk), f[f"{tag}/w/{rk}"], 1e-4, 2.5e-4, f"{tag} weight {k}")
    if sn is not None:
        for k, t in sn.items():
            assert_close(probe(t, k), f[f"{tag}/buf/{k}"], 1e-4, 1e-6, f"{tag} buffer {k}")


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 8), (128, 128, 4)])
def test_spectral_norm_steps(size, latent, batch):
    """oracle.d_step / g_step with ``sn`` (power iteration per training forward, gradient through sigma) against
    VanillaGAN(use_spectral_norm=True) run on the reference itself (make_golden.py::make_spectral_norm_steps)."""
    import os
    from common import GOLDEN, d_chans
    f = np.load(os.path.join(GOLDEN, "golden_sn_steps.npz"))
    tag = f"s{size}_b{batch}"
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, d_chans(size) * 2)]
    nb = len(masks) // 2
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, g_opt, d_opt, sn = oracle_states_sn(size, latent)
    met, grads = O.d_step(g_sd, d_sd, d_opt, real, z, masks[:nb], masks[nb:], size, signs=census_signs(f, f"{tag}/d"), sn=sn)
    _sn_check(f, f"{tag}/d", d_opt.names, DK + ("d_real_acc", "d_fake_acc"), met, grads, d_sd, d_opt, sn)
    met, grads = O.g_step(g_sd, d_sd, g_opt, z2, size, signs=census_signs(f, f"{tag}/g"), sn=sn)   # on the state the D step left (as the fixture)
    _sn_check(f, f"{tag}/g", g_opt.names, GK, met, grads, g_sd, g_opt)
    for k, t in sn.items():                                        # D.eval(): the buffers did not move
        assert_close(probe(t, k), f[f"{tag}/g/dbuf/{k}"], 1e-6, 1e-7, f"G step leaves {k} alone")
