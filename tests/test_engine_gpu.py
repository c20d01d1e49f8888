"""Parity of the HIP path (through the C ABI) against the oracle on the same seeded inputs and
against the golden fixtures (outputs of the reference).  Tolerances are fp32: the north star
asks for 1e-3; these assert 2e-4 relative to the tensor's scale for activations / losses /
gradients and bound Adam-updated weights by what one step can move ("Adam")."""
import numpy as np
import pytest
import torch

from common import (CASES, DK, GK, TIMED, I, O, SEED, assert_close, census_signs, d_chans, flips_vs_census, load_golden, masks_from,
                    oracle_states, oracle_states_sn, probe)

pytestmark = pytest.mark.gpu
RT = 2e-4
# what every step case measured: written next to the run (gpurun_out/parity_margins.json; the copy of the round's final
# binary is committed as profiles/r03_parity_margins.json): per case / tag / network the activation-sign decisions of the
# HIP path that differ from the REFERENCE run's (counted directly against the fixture's census, each one listed), which
# branch of the reference comparison ran (strict 1e-3, or "explained": HIP - reference = what those decisions produce), and
# the worst deviations of every link of the chain (_reference_chain)
MARGINS = {}


def _dump_margins():
    import json
    import os
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_margins.json"), "w") as f:
        json.dump(MARGINS, f, indent=1, sort_keys=True, default=float)


def _scale_close(got, want, what, rt=RT):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() + 1e-30
    err = np.abs(got - want).max()
    assert err <= rt * scale, f"{what}: max err {err:.3e}, scale {scale:.3e}"


def _forward_case(size, latent, batch, max_batch=None):
    from hipcommon import cuda, make_engine
    f, _ = load_golden(size, batch, latent)
    eng = make_engine(size, latent, max_batch or batch)
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    g_sd, d_sd, _, _ = oracle_states(size, latent, warm=False)

    img = eng.g_forward(cuda(z), training=False).cpu()
    _scale_close(img.numpy(), O.g_forward(g_sd, z, False, size).numpy(), "G eval vs oracle")
    flat = img.reshape(-1).numpy()
    _scale_close(flat[I.probe_idx(flat.size, "img", 256)], f["g_eval/probe"], "G eval vs golden")
    if "g_eval/img" in f:
        _scale_close(img.numpy(), f["g_eval/img"], "G eval full image vs golden")

    img = eng.g_forward(cuda(z), training=True).cpu()
    _scale_close(img.numpy(), O.g_forward(g_sd, z, True, size).numpy(), "G train vs oracle")
    flat = img.reshape(-1).numpy()
    _scale_close(flat[I.probe_idx(flat.size, "img", 256)], f["g_train/probe"], "G train vs golden")
    bn = eng.bn_views()
    for k, t in bn.items():
        _scale_close(probe(t.float().cpu(), k), f["g_train/buf/" + k], f"BN buffer {k} vs golden")
        _scale_close(t.float().cpu().numpy(), g_sd[k].float().numpy(), f"BN buffer {k} vs oracle")

    p, feat = eng.d_forward(cuda(real), training=False, want_features=True)
    _scale_close(p.cpu().reshape(-1).numpy(), f["d_eval/probs"], "D eval probs vs golden")
    _scale_close(feat.cpu().numpy(), O.d_features(d_sd, real, size).numpy(), "D features vs oracle")
    ff = feat.cpu().reshape(-1).numpy()
    _scale_close(ff[I.probe_idx(ff.size, "feat", 256)], f["d_eval/feat_probe"], "D features vs golden")
    masks = masks_from(f, "d_train/masks", batch, size, 1)
    p = eng.d_forward(cuda(real), training=True, masks=masks)
    _scale_close(p.cpu().reshape(-1).numpy(), f["d_train/probs"], "D train probs vs golden")
    eng.close()


@pytest.mark.parametrize("size,latent,batch", CASES)
def test_forward_vs_oracle_and_golden(size, latent, batch):
    _forward_case(size, latent, batch)


# A context created for more than 256 images (siggan_create: max_batch) runs Generator.fc -- generator_vanilla_gan.py:124-128 --
# through the generic kernels (k_fc_fwd / k_fc_wgrad + the column reductions + the k-major weight copy of k_prepare) instead of
# the one-launch MFMA kernels, whatever the batch of the call; so does a latent size that is not a multiple of 4 (CASES' last
# entry: z = 50 of the ablation grid, ablation_vanilla_gan_signatures.py:597).  Same fixtures, same bars.
BIG_CTX = 320


def test_forward_in_a_context_for_320_images():
    _forward_case(64, 100, 64, max_batch=BIG_CTX)


from hipcommon import count_sign_flips, grad_scales, hip_signs_d, hip_signs_g  # noqa: E402  (sign decisions of the HIP path, shared with smoke())

LR = 2e-4


def _adam_envelope(w0, m0, v0, g, tol, step, lr=LR):
    """[lo, hi] of the weight one torch-Adam update gives for ANY gradient within +-tol of g (elementwise; the update is
    evaluated at g - tol, g, g + tol).  A weight check that stays meaningful where Adam turns a gradient of rounding-noise
    size into a +-lr move ("Adam"): such an element's envelope is wide, every other element's is tight."""
    outs = []
    for d in (-tol, 0.0, tol):
        w, m, v = w0.clone(), m0.clone(), v0.clone()
        O.adam_update(w, g + d, m, v, step, lr, 0.5, 0.999)
        outs.append(w)
    st = torch.stack(outs)
    return st.amin(0) - 2e-3 * lr, st.amax(0) + 2e-3 * lr


class _Half:
    """Everything one half-step (D or G) left behind, on the CPU: metrics, gradients, moments, weights."""

    def __init__(self, met, grads, m, v, w, step):
        self.met, self.g, self.m, self.v, self.w, self.step = met, grads, m, v, w, step

    @classmethod
    def of_engine(cls, eng, which, met):
        gv, mv, vv, wv = (eng.views(which, a) for a in ("grads", "exp_avg", "exp_avg_sq", "params"))
        cp = lambda d: {k: t.detach().cpu().clone() for k, t in d.items()}
        steps = getattr(eng, f"{which}_adam_steps").cpu()
        assert float(steps.min()) == float(steps.max())
        return cls(met, cp(gv), cp(mv), cp(vv), cp(wv), float(steps[0]))

    @classmethod
    def of_oracle(cls, met, grads, sd, opt):
        return cls(met, grads, opt.m, opt.v, {k: sd[k] for k in opt.names}, float(opt.step))


def _scales(ref_grads, names, ref_gn):
    """Per-tensor comparison scale: the tensor's own largest gradient, floored at 1e-3 of the network's (a parameter whose
    true gradient is zero -- the Linear bias in front of BatchNorm1d -- holds rounding noise in every implementation, the
    reference included: floored at 1e-2)."""
    gscale = max(float(ref_grads[k].abs().max()) for k in names)
    noise = {k: bool(rn < 1e-5 * float(ref_gn.max())) for k, rn in zip(names, ref_gn)}
    return {k: max(float(ref_grads[k].abs().max()), (1e-2 if noise[k] else 1e-3) * gscale) for k in names}, noise


def _close_halves(a, b, names, scale, init_sd, init_opt, gtol, what):
    """a vs b, both complete half-steps: gradients / first moments within gtol of the tensor's scale, second moments within
    gtol of theirs, weights inside the Adam envelope of b's gradient +- gtol.  Returns the worst gradient error / scale."""
    worst = 0.0
    for k in names:
        err = float((a.g[k] - b.g[k]).abs().max()) / scale[k]
        worst = max(worst, err)
        assert err <= gtol, f"{what} grad {k}: {err:.3e} of scale {scale[k]:.3e}"
        assert float((a.m[k] - b.m[k]).abs().max()) <= gtol * scale[k], f"{what} exp_avg {k}"
        assert float((a.v[k] - b.v[k]).abs().max()) <= 2 * gtol * float(b.v[k].abs().max()) + 1e-12, f"{what} exp_avg_sq {k}"
        lo, hi = _adam_envelope(init_sd[k], init_opt.m[k], init_opt.v[k], b.g[k], gtol * scale[k], b.step)
        assert bool(((a.w[k] >= lo) & (a.w[k] <= hi)).all()), f"{what} weight {k} outside the Adam envelope"
    assert a.step == b.step
    return worst


def _golden_dev(h, f, tag, names, scale, noise):
    """Deviation of a half-step from the reference run's record: (grad-norm relative, grad probes / tensor scale, metrics)."""
    ref_gn = f[f"{tag}/grad_norm"]
    dn = {k: (float(h.g[k].norm()) - float(rn)) / float(rn) for k, rn in zip(names, ref_gn) if not noise[k]}
    dp = {k: (probe(h.g[k], k) - f[f"{tag}/grad/{k}"]) / scale[k] for k in names}
    dm = {}
    for k, v in h.met.items():
        if v is not None and f"{tag}/metric/{k}" in f:
            ref = float(f[f"{tag}/metric/{k}"])
            dm[k] = (v - ref) / (abs(ref) + 1e-2)
    return dn, dp, dm


def _golden_weights(h, f, tag, names, scale, init_sd, init_opt, gtol, what):
    for k in names:
        i = I.probe_idx(init_sd[k].numel(), k)
        pick = lambda t: t.reshape(-1)[torch.from_numpy(i)]
        lo, hi = _adam_envelope(pick(init_sd[k]), pick(init_opt.m[k]), pick(init_opt.v[k]), torch.from_numpy(f[f"{tag}/grad/{k}"]),
                                gtol * scale[k], h.step)
        w = torch.from_numpy(np.asarray(f[f"{tag}/w/{k}"]))
        assert bool(((pick(h.w[k]) >= lo) & (pick(h.w[k]) <= hi)).all()), f"{what} weight {k} vs the reference's gradient"
        assert bool(((w >= lo) & (w <= hi)).all()), f"{what}: the reference's own weight {k} outside its gradient's envelope"
    assert h.step == float(f[f"{tag}/adam_step"])


def _reference_chain(which, f, tag, step, eng, met, hip_signs, run_oracle, init_sd, init_opt, keep=None):
    """HIP vs the REFERENCE RUN, closed decision for decision:

      A = the HIP path                      B = oracle given the HIP path's activation-sign decisions
      G = the reference's record (fixture)  C = oracle given the REFERENCE run's decisions (the fixture's census)

    A = B to 1e-4 (arithmetic of the HIP path);  C = G to 1e-4 (the oracle IS the reference's arithmetic, on this host too);
    flips = the HIP decisions that differ from the reference run's, counted directly against the census.  With no flip A is
    held to G at the north star's 1e-3, no exceptions; with flips, A - G must be what those decisions alone produce, B - C, to
    1e-3 of scale -- nothing else may separate the HIP path from the reference."""
    names = list(eng.views(which, "grads"))
    A = _Half.of_engine(eng, which, met)
    rec = []
    B = _Half.of_oracle(*run_oracle(hip_signs, rec))
    n_vs_oracle = count_sign_flips(hip_signs, rec, keep=keep)        # asserts: every one within 1e-5 of the layer scale of zero
    C = _Half.of_oracle(*run_oracle(census_signs(f, step), None))
    flips = flips_vs_census(f, step, hip_signs, keep=keep)
    ref_gn = f[f"{tag}/grad_norm"]
    scale, noise = _scales(B.g, names, ref_gn)
    row = {"flips_vs_reference": len(flips), "flips": [{"layer": l, "index": i, "reference_value_over_layer_max": v} for l, i, v in flips],
           "sign_flips_hip_vs_own_oracle": n_vs_oracle}
    for k, v in B.met.items():
        if v is not None:
            assert_close(A.met[k], v, 2e-4, 2e-6, f"{tag} metric {k} vs oracle")
    row["hip_vs_oracle_with_hip_signs"] = _close_halves(A, B, names, scale, init_sd, init_opt, 1e-4, f"{tag} HIP vs oracle(HIP signs)")
    # C vs G: on THIS host's CPU (the GPU box), whatever its thread count
    cn, cp, cm = _golden_dev(C, f, tag, names, scale, noise)
    row["oracle_with_reference_signs_vs_reference"] = max([abs(x) for x in cn.values()] + [float(np.abs(x).max()) for x in cp.values()])
    assert row["oracle_with_reference_signs_vs_reference"] <= 1e-4, (tag, "oracle(reference's signs) does not reproduce the fixture", row)
    assert all(abs(x) <= 2e-4 for x in cm.values()), (tag, cm)
    _golden_weights(C, f, tag, names, scale, init_sd, init_opt, 1e-4, f"{tag} oracle(reference signs)")
    an, ap, am = _golden_dev(A, f, tag, names, scale, noise)
    bn, bp, _ = _golden_dev(B, f, tag, names, scale, noise)
    fwd = {k: v for k, v in am.items() if not k.endswith("grad_norm")}
    row["metric_vs_reference"] = max(abs(x) for x in fwd.values())
    assert row["metric_vs_reference"] <= 2e-4, (tag, fwd)             # losses / predictions: the forward pass, no decision involved
    row["grad_norm_vs_reference"] = max(abs(x) for x in an.values())
    row["grad_probe_vs_reference"] = max(float(np.abs(x).max()) for x in ap.values())
    if not flips:
        row["branch"] = "strict 1e-3 (no decision differs from the reference run)"
        assert row["grad_norm_vs_reference"] <= 1e-3 and row["grad_probe_vs_reference"] <= 1e-3, (tag, row)
        assert all(abs(x) <= 1e-3 for x in am.values()), (tag, am)
        _golden_weights(A, f, tag, names, scale, init_sd, init_opt, 1e-3, f"{tag} HIP")
    else:
        # what the differing decisions alone produce: oracle(HIP signs) - oracle(reference signs); A - G must equal it
        cnv = {k: (float(C.g[k].norm()) - float(rn)) / float(rn) for k, rn in zip(names, ref_gn) if not noise[k]}
        pred_n = {k: bn[k] - cnv[k] for k in bn}
        pred_p = {k: bp[k] - cp[k] for k in names}
        row["predicted_by_the_flips_grad_norm"] = max(abs(x) for x in pred_n.values())
        row["predicted_by_the_flips_grad_probe"] = max(float(np.abs(x).max()) for x in pred_p.values())
        row["residual_grad_norm"] = max(abs(an[k] - pred_n[k]) for k in an)
        row["residual_grad_probe"] = max(float(np.abs(ap[k] - pred_p[k]).max()) for k in names)
        row["branch"] = f"explained by {len(flips)} decision(s): HIP - reference = oracle(HIP signs) - oracle(reference signs) to 1e-3"
        assert row["residual_grad_norm"] <= 1e-3 and row["residual_grad_probe"] <= 1e-3, (tag, row)
    return row


def _single_steps(size, latent, batch, tag, max_batch=None):
    from hipcommon import cuda, make_engine
    f, meta = load_golden(size, batch, latent)
    key = f"s{size}_b{batch}" + ("" if latent in (100, 128) else f"_z{latent}") + (f"_ctx{max_batch}" if max_batch else "")
    max_batch = max_batch or batch
    clip = meta["clip"] if tag == "clip" else None
    warm = tag != "fresh"
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    masks = masks_from(f, f"dstep_{tag}/masks", batch, size, 2)
    nb = len(masks) // 2

    # ---- D step ------------------------------------------------------------------------
    eng = make_engine(size, latent, max_batch, warm=warm)
    met = eng.d_step(cuda(real), cuda(z), masks, clip=clip)

    def oracle_d(signs, rec):
        g_sd, d_sd, _, d_opt = oracle_states(size, latent, warm=warm)
        o_met, o_grads = O.d_step(g_sd, d_sd, d_opt, real, z, masks[:nb], masks[nb:], size, clip=clip, signs=signs, record=rec)
        return o_met, o_grads, d_sd, d_opt
    _, i_d, _, i_dopt = oracle_states(size, latent, warm=warm)
    MARGINS[f"{key}/{tag}/d"] = _reference_chain("d", f, f"dstep_{tag}", "dstep", eng, met, hip_signs_d(eng, size, batch, 2),
                                                            oracle_d, i_d, i_dopt, keep=masks)
    _dump_margins()
    eng.close()

    # ---- G step ------------------------------------------------------------------------
    eng = make_engine(size, latent, max_batch, warm=warm)
    met = eng.g_step(batch, cuda(z2), clip=clip)
    bufs = {}

    def oracle_g(signs, rec):
        g_sd, d_sd, g_opt, _ = oracle_states(size, latent, warm=warm)
        o_met, o_grads = O.g_step(g_sd, d_sd, g_opt, z2, size, clip=clip, signs=signs, record=rec)
        bufs.update({k: v for k, v in g_sd.items() if k not in g_opt.names})
        return o_met, o_grads, g_sd, g_opt
    i_g, _, i_gopt, _ = oracle_states(size, latent, warm=warm)
    MARGINS[f"{key}/{tag}/g"] = _reference_chain("g", f, f"gstep_{tag}", "gstep", eng, met,
                                                            hip_signs_g(eng, size, batch) + hip_signs_d(eng, size, batch, 1),
                                                            oracle_g, i_g, i_gopt)
    _dump_margins()
    for k, t in eng.bn_views().items():
        _scale_close(probe(t.float().cpu(), k), f[f"gstep_{tag}/buf/{k}"], f"gstep BN buffer {k} vs golden")
    eng.close()


@pytest.mark.parametrize("size,latent,batch", CASES)
@pytest.mark.parametrize("tag", ["warm", "fresh", "clip"])
def test_single_steps(size, latent, batch, tag):
    _single_steps(size, latent, batch, tag)


@pytest.mark.parametrize("tag", ["warm", "clip"])
def test_single_steps_in_a_context_for_320_images(tag):
    _single_steps(64, 100, 64, tag, max_batch=BIG_CTX)


from hipcommon import oracle_state_of as _oracle_state_of  # noqa: E402  (shared with test_timed_step_gpu)


def _grads_close(eng, which, o_grads, what, tol=1e-4):
    """HIP gradient arena vs an oracle's, each tensor relative to its own scale (hipcommon.grad_scales)."""
    gv = eng.views(which, "grads")
    scale = grad_scales(o_grads, list(gv))
    worst = 0.0
    for k, t in gv.items():
        err = float((t.cpu() - o_grads[k]).abs().max()) / scale[k]
        worst = max(worst, err)
        assert err <= tol, f"{what} grad {k}: {err:.3e} of scale {scale[k]:.3e}"
    return worst


SEQ3_RT, SEQ3_AT = 1e-3, 1e-4        # the north star's 1e-3 on the chained metrics (losses / mean predictions, O(0.1 .. 1))


@pytest.mark.parametrize("size,latent,batch", CASES)
def test_three_step_sequence(size, latent, batch):
    """VanillaGAN.train_step three times over (vanilla_gan_model.py:308-336), closed like the single steps:

      per half-step   the HIP gradients equal oracle(the HIP path's sign decisions) run FROM THE ENGINE'S OWN STATE before that
                      half-step, to 1e-4 of the tensor's scale, metrics to 2e-4 -- the arithmetic of every chained step;
      the sequence    A = the HIP metrics, G = the reference's record, C = the oracle chain given the reference run's decisions
                      (the fixture's per-half-step census; C = G to 1e-4 is asserted here and on the CPU), B = the oracle chain
                      given the HIP path's decisions.  No differing decision: A = G at 1e-3, strictly.  Otherwise A - G must be
                      what those decisions produce, B - C, to the same 1e-3 -- the bare 1e-2 of round 3 is gone."""
    from hipcommon import cuda, make_engine
    f, _ = load_golden(size, batch, latent)
    real_c = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    real = cuda(real_c)
    eng = make_engine(size, latent, batch, warm=True)
    masks = masks_from(f, "seq3/masks", batch, size, 6)
    nb = len(masks) // 6
    Bc, Cc = oracle_states(size, latent, warm=True), oracle_states(size, latent, warm=True)     # (g_sd, d_sd, g_opt, d_opt)
    rows = {"A": [], "B": [], "C": []}
    nflips, worst = 0, 0.0
    dk = ("d_loss", "d_loss_real", "d_loss_fake", "d_real_mean", "d_fake_mean")
    gk = ("g_loss", "g_fake_mean")
    for s in range(3):
        zs_c, zg_c = (torch.from_numpy(I.gen_z(batch, latent, 1000 + 2 * s + j)) for j in (0, 1))
        ms = masks[2 * nb * s: 2 * nb * (s + 1)]
        # ---- D half ----
        g0, d0, _, do0 = _oracle_state_of(eng, size, latent)
        dm = eng.d_step(real, cuda(zs_c), ms)
        hs = hip_signs_d(eng, size, batch, 2)
        rec = []
        om, og = O.d_step(g0, d0, do0, real_c, zs_c, ms[:nb], ms[nb:], size, signs=hs, record=rec)
        count_sign_flips(hs, rec, keep=ms)
        for k in dk:
            assert_close(dm[k], om[k], 2e-4, 2e-6, f"step {s} D metric {k} vs oracle(HIP signs) from the engine's state")
        worst = max(worst, _grads_close(eng, "d", og, f"step {s} D"))
        bm, _ = O.d_step(Bc[0], Bc[1], Bc[3], real_c, zs_c, ms[:nb], ms[nb:], size, signs=hs)
        cm, _ = O.d_step(Cc[0], Cc[1], Cc[3], real_c, zs_c, ms[:nb], ms[nb:], size, signs=census_signs(f, f"seq3/d{s}"))
        nflips += len(flips_vs_census(f, f"seq3/d{s}", hs, keep=ms))
        # ---- G half ----
        g0, d0, go0, _ = _oracle_state_of(eng, size, latent)
        gm = eng.g_step(batch, cuda(zg_c))
        hs = hip_signs_g(eng, size, batch) + hip_signs_d(eng, size, batch, 1)
        rec = []
        om, og = O.g_step(g0, d0, go0, zg_c, size, signs=hs, record=rec)
        count_sign_flips(hs, rec)
        for k in gk:
            assert_close(gm[k], om[k], 2e-4, 2e-6, f"step {s} G metric {k} vs oracle(HIP signs) from the engine's state")
        worst = max(worst, _grads_close(eng, "g", og, f"step {s} G"))
        bg, _ = O.g_step(Bc[0], Bc[1], Bc[2], zg_c, size, signs=hs)
        cg, _ = O.g_step(Cc[0], Cc[1], Cc[2], zg_c, size, signs=census_signs(f, f"seq3/g{s}"))
        nflips += len(flips_vs_census(f, f"seq3/g{s}", hs))
        for name, d_, g_ in (("A", dm, gm), ("B", bm, bg), ("C", cm, cg)):
            rows[name].append([d_[k] for k in dk] + [g_[k] for k in gk])
    A, B, Cm = (np.array(rows[k], np.float64) for k in "ABC")
    G = np.asarray(f["seq3/metrics"], np.float64)
    assert_close(Cm, G, 1e-4, 1e-5, "3-step metrics: oracle(reference's decisions) vs the reference")
    row = {"flips_vs_reference": nflips, "hip_vs_oracle_with_hip_signs": worst,
           "metrics_vs_reference": float(np.abs(A - G).max()), "predicted_by_the_flips": float(np.abs(B - Cm).max())}
    if nflips == 0:
        row["branch"] = "strict 1e-3 (no decision differs from the reference run)"
        assert_close(A, G, SEQ3_RT, SEQ3_AT, "3-step metrics vs the reference")
    else:
        row["branch"] = f"explained by {nflips} decision(s): HIP - reference = oracle(HIP signs) - oracle(reference signs) to 1e-3"
        row["residual"] = float(np.abs((A - G) - (B - Cm)).max())
        assert_close(A - (B - Cm), G, SEQ3_RT, SEQ3_AT, "3-step metrics vs the reference, the differing decisions' effect removed")
    MARGINS[f"s{size}_b{batch}" + ("" if latent in (100, 128) else f"_z{latent}") + "/seq3"] = row
    _dump_margins()
    eng.close()


def test_execution_modes_are_bitwise_identical(dtype="f32", size=64, latent=100, batch=16):
    """hipGraph replay and side-stream overlap only change scheduling: with injected noise and
    masks the four mode combinations must give bit-identical parameters, moments and metrics,
    also on the replayed (second and third) steps."""
    from hipcommon import cuda, make_engine
    real = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"])))
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, d_chans(size) * 2, 3)]
    ref = None
    for graph, overlap, pipelined in ((False, False, False), (True, True, False), (True, False, False), (False, True, False),
                                      (False, True, True), (False, False, True)):
        eng = make_engine(size, latent, batch, warm=True, dtype=dtype)
        eng.set_mode(graph=graph, overlap=overlap)
        mets = []
        for s in range(3):
            z1 = cuda(torch.from_numpy(I.gen_z(batch, latent, 50 + s)))
            z2 = cuda(torch.from_numpy(I.gen_z(batch, latent, 60 + s)))
            if pipelined:        # siggan_step_begin: the G step's forward runs beside the D step's backward
                m = eng.train_step(real, z1, masks, z2, clip=0.5)
                mets.append({k: v for k, v in m.items() if k.startswith("d_")})
                mets.append({k: v for k, v in m.items() if k.startswith("g_")})
            else:
                mets.append(eng.d_step(real, z1, masks, clip=0.5))
                mets.append(eng.g_step(batch, z2, clip=0.5))
        state = [t.clone() for t in (eng.g_params, eng.d_params, eng.g_exp_avg_sq, eng.d_exp_avg, eng.g_bn_mean, eng.g_bn_var,
                                     eng.g_adam_steps, eng.g_bn_batches)]
        eng.close()
        if ref is None:
            ref = (state, mets)
        else:
            for a, b in zip(ref[0], state):
                assert torch.equal(a, b), f"mode graph={graph} overlap={overlap} pipelined={pipelined} changed the result"
            assert mets == ref[1]


@pytest.mark.parametrize("dtype,size,latent,batch", [t for t in TIMED if t[0] == "f32"])
def test_execution_modes_are_bitwise_identical_at_timed_shapes(dtype, size, latent, batch):
    """The same at the fp32 workloads bench.py times: tile / split-K choice, the classifier in the split-K epilogue and the
    number of k_adam_pack's riders (B * S/4: 1024, 2048 and 4096 here) all depend on the batch."""
    test_execution_modes_are_bitwise_identical(dtype, size, latent, batch)


def test_debug_hooks_follow_a_replayed_g_step(size=64, latent=100):
    """What a G step leaves behind for siggan_debug_tensor -- the first workspace row of its Discriminator pass ('d_a_g') and
    the batch whose last Generator activation was not materialised ('g_a'[Lg]) -- is committed on every graph replay, not only
    when the phase is captured: after G steps at batch 4, 5, an eval forward at batch 4 and a G step at batch 4, the hooks and
    the arenas must be bit for bit what the eager engine leaves.  That fourth call is still a first capture (the eval forward
    cleared the 'packs are stale' flags, which are part of the graph key), so calls 2-4 are made a second time, as replays of
    graphs captured in the first round, and the hooks are also read right after the replayed batch-5 step, at batch 5: the
    last capture before it was a batch-4 step, so state left by a capture alone reads from row 4 and forms 4 images there."""
    from hipcommon import cuda, make_engine
    zs = [cuda(torch.from_numpy(I.gen_z(b, latent, 70 + i))) for i, b in enumerate((4, 5, 4, 4))]
    a, b = engs = [make_engine(size, latent, 5, warm=True) for _ in range(2)]
    a.set_mode(graph=True, overlap=False)
    b.set_mode(graph=False, overlap=False)
    lg = len(O.G_CHAIN[size]) - 1

    def same_hooks(batch, where):
        for l, c in enumerate(O.D_CHAIN[size], start=1):
            shape = (batch, size >> l, size >> l, c)
            assert torch.equal(a.debug_tensor("d_a_g", l, shape), b.debug_tensor("d_a_g", l, shape)), (where, "d_a_g", l)
        shape = (batch, size, size, 32)
        assert torch.equal(a.debug_tensor("g_a", lg, shape), b.debug_tensor("g_a", lg, shape)), (where, "g_a")

    for rnd in range(2):
        for eng in engs:
            if rnd == 0:
                eng.g_step(4, zs[0])
            eng.g_step(5, zs[1])
        if rnd == 1:
            same_hooks(5, "replayed batch-5 step")
        for eng in engs:
            eng.g_forward(zs[2], training=False)
            eng.g_step(4, zs[3])
        same_hooks(4, f"round {rnd}, batch-4 step")
        for n in ("g_params", "d_params", "g_exp_avg", "g_exp_avg_sq", "d_exp_avg", "d_exp_avg_sq"):
            assert torch.equal(getattr(a, n), getattr(b, n)), (rnd, n)
    for eng in engs:
        eng.close()


@pytest.mark.parametrize("dtype,size,latent,batch", [("f32", 64, 100, 16), ("bf16", 64, 100, 16), ("f32", 128, 128, 4)] + TIMED)
def test_update_launch_leaves_the_packs_the_prepare_pass_would(dtype, size, latent, batch):
    """k_adam_pack (the optimiser update that also writes the MFMA weight packs, the permuted one-channel weights and the
    BatchNorm eval tables) against k_prepare: after pipelined steps -- whose updates wrote them, the D one with the next
    pass' first block riding along at fp32 -- every pass that reads a pack must give the bits it gives once
    siggan_params_changed has forced the prepare pass to rebuild them from the same arena: both forwards (forward packs,
    tables, tap-major copies, the classifier's permutation) and the G step's gradients (both networks' input-gradient packs)."""
    from hipcommon import cuda, make_engine
    reals = [cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + t))) for t in range(3)]
    z = cuda(torch.from_numpy(I.gen_z(batch, latent, 91)))

    def run(rebuild):
        eng = make_engine(size, latent, batch, warm=True, dtype=dtype)
        eng.seed(77)
        for t in range(2):
            eng.train_step(reals[t], clip=0.5 if t else None, next_real=reals[t + 1])
        if rebuild:
            eng.params_changed()
        img = eng.g_forward(z, training=False).clone()
        pr = eng.d_forward(reals[2]).clone()
        eng.g_compute_grads(batch, z)
        out = img, pr, eng.g_grads.clone(), eng.d_params.clone()
        eng.close()
        return out

    a, b = run(False), run(True)
    for name, x, y in zip(("generated images", "D(real) predictions", "G-step gradients", "D parameters"), a, b):
        assert torch.equal(x, y), f"{name}: the packs written by the update launch differ from the prepare pass'"


def test_staged_next_batch_is_bitwise_identical(dtype="f32", size=64, latent=100, batch=16):
    """siggan_stage_real: D(real) of step t+1 runs beside the Generator backward of step t.  With the
    library's own RNG (z and dropout drawn on the device) the staged sequence must reproduce the
    un-staged one bit for bit -- parameters, Adam moments, BatchNorm statistics and every metric --
    including when a staged batch is dropped (different tensor passed) or the weights are touched."""
    from hipcommon import cuda, make_engine
    reals = [cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + 7 * t))) for t in range(5)]

    def run(kind):
        eng = make_engine(size, latent, batch, warm=True, dtype=dtype)
        eng.seed(1234)
        mets = []
        for t in range(4):
            nxt = reals[t + 1] if kind != "plain" else None
            if kind == "dropped" and t == 1:
                nxt = reals[4]                      # staged batch that the next step does not use
            mets.append(eng.train_step(reals[t], clip=0.5, next_real=nxt))
            if kind == "touched" and t == 2:
                eng.params_changed()                # forces the D(real) forward started ahead of time to be redone
        state = [x.clone() for x in (eng.g_params, eng.d_params, eng.g_exp_avg, eng.d_exp_avg_sq, eng.g_bn_mean, eng.g_bn_var)]
        eng.close()
        return state, mets

    ref_state, ref_mets = run("plain")
    for kind in ("staged", "dropped", "touched"):
        state, mets = run(kind)
        assert mets == ref_mets, kind
        for a, b in zip(ref_state, state):
            assert torch.equal(a, b), f"{kind}: staging the next batch changed the result"


@pytest.mark.parametrize("dtype,size,latent,batch", TIMED)
def test_staged_next_batch_is_bitwise_identical_at_timed_shapes(dtype, size, latent, batch):
    test_staged_next_batch_is_bitwise_identical(dtype, size, latent, batch)


@pytest.mark.parametrize("dtype,size,latent,batch", TIMED)
def test_timed_loop_is_bitwise_the_pipelined_and_the_split_steps(dtype, size, latent, batch):
    """bench.py's loop as it is written -- DataParallelStep(eng) at world 1 with no process group, step(real, next_real=real),
    sync=False, library RNG, bench.py's engine and starting state -- bit for bit against the same engine and seed run
    (a) as the unstaged pipelined step (step_begin / d_apply / g_compute_grads / g_apply, no next batch) and
    (b) as split steps, d_step(real) + g_step(batch, z_g), over four steps: parameters, both Adam moments and step counts,
    BatchNorm buffers and all 16 metrics after every step.

    (b) draws its own z and dropout tables but is handed the Generator step's z_g that (a) drew: split and pipelined steps
    do not draw the same latent batch, by design.  The fc kernel draws z at the RNG counter in force when the Generator's
    training forward runs, and the counter ticks once per optimiser update; the pipelined step runs that forward in
    siggan_step_begin, before the D update (counter t), g_step after it (t + 1).  Everything else is drawn at the same
    counter on both paths -- including the dropout tables of a staged D(real) pass, which the previous G step draws one
    update ahead (make_noise's ctr_add = 1) -- and that is what (a) against the timed loop checks."""
    from hipcommon import bench_setup, debug_scalar, full_state, assert_same_state
    steps = 4
    eng, dp, real = bench_setup(dtype, size, latent, batch)
    timed = []
    for _ in range(steps):
        dp.step(real, next_real=real)
        timed.append(full_state(eng))
    assert debug_scalar(eng, "pre_real") == batch              # the loop staged: it is not the unstaged one below
    eng.close()

    hp = dp.hp
    eng, dp, real = bench_setup(dtype, size, latent, batch)
    z_g = []
    for s in range(steps):
        eng.step_begin(real, label_smoothing=hp["ls"])
        eng.d_apply(hp["lr_d"], hp["beta1"], hp["beta2"], sync=False)
        eng.g_compute_grads(batch)
        z_g.append(eng.debug_tensor("z_g", 0, (batch, latent)).clone())
        eng.g_apply(hp["lr_g"], hp["beta1"], hp["beta2"], sync=False)
        assert debug_scalar(eng, "pre_real") == 0
        assert_same_state(timed[s], full_state(eng), f"step {s}: the timed loop vs the unstaged pipelined step")
    eng.close()

    eng, dp, real = bench_setup(dtype, size, latent, batch)
    for s in range(steps):
        eng.d_step(real, sync=False)
        eng.g_step(batch, z_g[s], sync=False)
        assert_same_state(timed[s], full_state(eng), f"step {s}: the timed loop vs split steps")
    eng.close()


def test_latent_drawn_inside_the_fc_kernel():
    """Without an explicit z the fc kernel draws the latent batch itself (no separate RNG launch) and leaves it in the
    workspace for the backward pass: it must be standard normal, and feeding the same values back as an explicit z must
    reproduce the step bit for bit."""
    from hipcommon import cuda, make_engine
    size, latent, batch = 64, 100, 64
    e1 = make_engine(size, latent, batch, warm=True)
    e1.seed(99)
    m1 = e1.g_step(batch, clip=0.5)
    z = e1.debug_tensor("z", 0, (batch, latent)).clone()
    assert torch.isfinite(z).all() and abs(float(z.mean())) < 0.05 and abs(float(z.std()) - 1.0) < 0.05
    assert float(z.abs().max()) < 6.0 and len(torch.unique(z)) > 0.99 * z.numel()
    e2 = make_engine(size, latent, batch, warm=True)
    e2.seed(99)
    m2 = e2.g_step(batch, z, clip=0.5)
    assert m1 == m2
    for a, b in zip((e1.g_params, e1.g_exp_avg_sq, e1.g_bn_mean), (e2.g_params, e2.g_exp_avg_sq, e2.g_bn_mean)):
        assert torch.equal(a, b)
    e1.close(); e2.close()


def test_one_sample_is_refused_where_torch_refuses_it():
    """generator_vanilla_gan.py:112: the fc block's BatchNorm1d in training mode refuses a batch of one ("Expected more than
    1 value per channel when training", a ValueError).  Same refusal, same exception type, at the same point of a step: the
    D step of a one-sample batch runs (G.eval(), no BatchNorm in D), the G step raises and leaves the Generator untouched;
    eval-mode generation and scoring of a single image work."""
    from hipcommon import cuda, make_engine
    size, latent = 64, 100
    eng = make_engine(size, latent, 4, warm=True)
    eng.seed(5)
    z = cuda(torch.randn(1, latent, generator=torch.Generator().manual_seed(1)))
    real = cuda(torch.from_numpy(I.gen_real(1, size, SEED["real"])))
    img = eng.g_forward(z, training=False)
    assert tuple(img.shape) == (1, 1, size, size) and torch.isfinite(img).all()
    assert torch.isfinite(eng.d_forward(real, training=False)).all()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        eng.g_forward(z, training=True)
    g_before, d_before = eng.g_params.clone(), eng.d_params.clone()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        eng.train_step(real, clip=0.5)                                    # D half done, G half refused (train...py:309-360)
    assert torch.equal(eng.g_params, g_before) and not torch.equal(eng.d_params, d_before)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        eng.g_step(1)
    met = eng.d_step(real, clip=0.5)                                      # the context is still usable
    assert all(v == v for v in met.values() if isinstance(v, float))
    eng.close()


def test_abandoned_staged_forward_is_ordered(dtype="f32", size=64, latent=100, batch=16):
    """A D(real) forward started ahead of time (siggan_stage_real) that no D step consumes must not race with what
    follows: a Discriminator forward on other images right behind the step, then a step on a DIFFERENT batch, give
    exactly what the un-staged sequence gives (the abandoned lane is waited for before its rows / packs are reused)."""
    from hipcommon import cuda, make_engine
    reals = [cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + 3 * t))) for t in range(3)]
    probe_x = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"] + 99)))

    def run(staged):
        eng = make_engine(size, latent, batch, warm=True, dtype=dtype)
        eng.seed(77)
        out = [eng.train_step(reals[0], clip=0.5, next_real=reals[1] if staged else None)]
        out.append(eng.d_forward(probe_x, training=False).clone())       # abandons the forward of reals[1]
        out.append(eng.train_step(reals[2], clip=0.5, next_real=reals[1] if staged else None))
        other = reals[0].clone()                                          # a different tensor: the staged one is dropped
        out.append(eng.train_step(other, clip=0.5))
        state = [x.clone() for x in (eng.g_params, eng.d_params, eng.d_exp_avg_sq, eng.g_bn_var)]
        eng.close()
        return out, state

    (m0, p0, m1, m2), s0 = run(False)
    (n0, q0, n1, n2), s1 = run(True)
    assert m0 == n0 and m1 == n1 and m2 == n2
    assert torch.equal(p0, q0)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype,size,latent,batch", TIMED)
def test_abandoned_staged_forward_is_ordered_at_timed_shapes(dtype, size, latent, batch):
    test_abandoned_staged_forward_is_ordered(dtype, size, latent, batch)


def test_rng_position_survives_a_larger_batch_and_is_readable():
    """Engine.ensure_batch re-creates the context for a larger batch: the z / dropout stream must continue (same seed,
    same call counter), not rewind to step 0."""
    from hipcommon import cuda, make_engine
    size, latent, batch = 64, 100, 8
    real = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"])))
    eng = make_engine(size, latent, batch, warm=True)
    eng.seed(4321)
    eng.train_step(real)
    eng.train_step(real)
    seed, off = eng.rng_state()
    assert seed == 4321 and off == 4                    # one tick per optimiser update
    eng.g_forward(torch.zeros(2 * batch, latent, device="cuda:0"))      # grows the workspace
    assert eng.max_batch == 2 * batch and eng.rng_state() == (4321, 4)
    eng.close()


def _rel_grads(eng, which, o_grads, ref_gn):
    """worst gradient error of the HIP path against an oracle run, relative to the tensor's scale (floored as in _scales)"""
    gv = eng.views(which, "grads")
    scale, _ = _scales(o_grads, list(gv), ref_gn)
    return max(float((gv[k].cpu() - o_grads[k]).abs().max()) / scale[k] for k in gv), scale


def _weights_in_envelope(eng, which, o_grads, scale, init_sd, init_opt, tol, step, what):
    """every weight inside what one torch-Adam update gives for a gradient within tol of the oracle's (see _adam_envelope)"""
    wv = eng.views(which, "params")
    for k in wv:
        lo, hi = _adam_envelope(init_sd[k], init_opt.m[k], init_opt.v[k], o_grads[k], tol * scale[k], step)
        w = wv[k].cpu()
        assert bool(((w >= lo) & (w <= hi)).all()), f"{what} weight {k} outside the Adam envelope"


def _golden_rel(f, tag, grads, names, scale, ren=lambda k: k):
    """worst deviation of a run's gradients from the reference's record: probes / tensor scale and relative norms"""
    gn = f[f"{tag}/grad_norm"]
    live = gn > 1e-5 * float(gn.max())
    dn = max(abs(float(grads[k].norm()) - float(r)) / float(r) for k, r, lv in zip(names, gn, live) if lv)
    dp = max(float(np.abs(probe(grads[k], ren(k)) - f[f"{tag}/grad/{ren(k)}"]).max()) / scale[k] for k in names)
    return max(dn, dp)


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 8), (128, 128, 4)])
def test_ablation_step_variant(size, latent, batch):
    """siggan_set_step_variant(SIGGAN_STEP_ABLATION): AblationGANTrainer.train_epoch's iteration
    (ablation_vanilla_gan_signatures.py:397-467) -- both nets in train mode, one shared Generator forward, G target = smoothed
    label, three dropout mask sets.  Same chain as test_single_steps: HIP vs the oracle given the HIP path's activation-sign
    decisions (arithmetic), the oracle given the REFERENCE replay's decisions (fixture census) vs the fixture, and the HIP
    decisions that differ from the replay's counted against the census."""
    import os
    from common import GOLDEN, ablation_groups
    from hipcommon import cuda, hip_ablation_iteration, make_engine
    f = np.load(os.path.join(GOLDEN, "golden_ablation_step.npz"))
    tag = f"s{size}_b{batch}"
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, d_chans(size) * 3)]
    nb = len(masks) // 3
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    eng = make_engine(size, latent, batch, warm=True)
    eng.set_step_variant("ablation")
    met, hip, keep, d_grads_hip, _, _ = hip_ablation_iteration(eng, real, z, masks, size, batch)

    def run(signs, rec):
        g_sd, d_sd, g_opt, d_opt = oracle_states(size, latent, warm=True)
        o = O.ablation_step(g_sd, d_sd, g_opt, d_opt, real, z, masks[:nb], masks[nb:2 * nb], masks[2 * nb:], size, signs=signs, record=rec)
        return o, g_sd, d_sd, g_opt, d_opt
    rec = {}
    (o_met, o_dg, o_gg), g_sd, d_sd, g_opt, d_opt = run(hip, rec)
    for grp in ("g", "d_real", "d_fake", "d_g"):
        count_sign_flips(hip[grp], rec[grp], keep=keep[grp])           # every disagreement within 1e-5 of the layer scale of zero
    for k, v in o_met.items():
        assert_close(met[k], v, 2e-4, 2e-6, f"ablation metric {k} vs oracle")
        key = f"{tag}/{k[0]}/metric/{k}"
        if key in f:
            assert_close(met[k], f[key], 2e-4, 2e-6, f"ablation metric {k} vs golden")
    row = {}
    gv = eng.views("g", "grads")
    sc_d, _ = _scales(o_dg, list(o_dg), f[f"{tag}/d/grad_norm"])
    row["hip_vs_oracle_with_hip_signs_d"] = max(float((d_grads_hip[k] - o_dg[k]).abs().max()) / sc_d[k] for k in o_dg)
    row["hip_vs_oracle_with_hip_signs_g"], sc_g = _rel_grads(eng, "g", o_gg, f[f"{tag}/g/grad_norm"])
    assert row["hip_vs_oracle_with_hip_signs_d"] <= 2e-4 and row["hip_vs_oracle_with_hip_signs_g"] <= 1e-4, row      # measured: 5.7e-5 / 7.7e-6
    i_g, i_d, i_gopt, i_dopt = oracle_states(size, latent, warm=True)
    for which, og, oopt, sc, isd, iopt in (("d", o_dg, d_opt, sc_d, i_d, i_dopt), ("g", o_gg, g_opt, sc_g, i_g, i_gopt)):
        mv = eng.views(which, "exp_avg")
        for k in mv:
            assert float((mv[k].cpu() - oopt.m[k]).abs().max()) <= 2e-4 * sc[k], (which, k, "exp_avg")
        _weights_in_envelope(eng, which, og, sc, isd, iopt, 2e-4, oopt.step, f"ablation {which}")
    # the reference replay's own decisions -> the fixture, on this host
    census = census_signs(f, tag)
    (c_met, c_dg, c_gg), *_ = run(ablation_groups(size, census), None)
    row["oracle_with_reference_signs_vs_reference"] = max(_golden_rel(f, f"{tag}/d", c_dg, list(c_dg), sc_d), _golden_rel(f, f"{tag}/g", c_gg, list(c_gg), sc_g))
    assert row["oracle_with_reference_signs_vs_reference"] <= 1e-4, row
    order = hip["d_real"] + hip["g"] + hip["d_fake"] + hip["d_g"]              # the harness' call order = the census' order
    flips = flips_vs_census(f, tag, order, keep=list(masks[:nb]) + [None] * len(hip["g"]) + list(masks[nb:]))
    row["flips_vs_reference"] = len(flips)
    row["hip_vs_reference"] = max(_golden_rel(f, f"{tag}/d", d_grads_hip, list(o_dg), sc_d),
                                  _golden_rel(f, f"{tag}/g", {k: v.cpu() for k, v in gv.items()}, list(o_gg), sc_g))
    pred = max(_golden_rel(f, f"{tag}/d", o_dg, list(o_dg), sc_d), _golden_rel(f, f"{tag}/g", o_gg, list(o_gg), sc_g))
    row["predicted_by_the_flips"] = pred
    if not flips:
        assert row["hip_vs_reference"] <= 1e-3, row
    else:
        assert abs(row["hip_vs_reference"] - pred) <= 1e-3, row
    MARGINS[f"ablation/{tag}"] = row
    _dump_margins()
    for k, t in eng.bn_views().items():
        _scale_close(probe(t.float().cpu(), k), f[f"{tag}/g/buf/{k}"], f"ablation BN buffer {k} vs golden")
    # the trainer step must be unaffected once the variant is switched back
    eng.set_step_variant("trainer")
    m2 = eng.train_step(cuda(real))
    assert np.isfinite(m2["d_loss"]) and np.isfinite(m2["g_loss"])
    eng.close()


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 8), (128, 128, 4)])
def test_spectral_norm_training(size, latent, batch):
    """Engine(spectral_norm=True): one D step then one G step (trainer variant) against the oracle's restatement of torch's
    spectral-norm hook and against VanillaGAN(use_spectral_norm=True) run on the reference itself -- power iteration per
    training forward (different effective weights for the real and the fake pass), gradient through sigma, u / v buffers.
    The oracle is given the HIP path's sign decisions (arithmetic) resp. the reference run's (fixture census), as in
    test_single_steps; the G step runs on the state the D step left, in the engine and in both oracle runs."""
    import os
    from common import GOLDEN
    from hipcommon import cuda, load_engine_state
    from signature_gan_amd.engine import Engine
    f = np.load(os.path.join(GOLDEN, "golden_sn_steps.npz"))
    tag = f"s{size}_b{batch}"
    masks = [torch.from_numpy(m) for m in I.unpack_masks(f[f"{tag}/masks"], batch, d_chans(size) * 2)]
    nb = len(masks) // 2
    z = torch.from_numpy(I.gen_z(batch, latent, SEED["z"]))
    z2 = torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1))
    real = torch.from_numpy(I.gen_real(batch, size, SEED["real"]))
    eng = load_engine_state(Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", spectral_norm=True),
                            size, latent, warm=True)
    _, _, _, _, sn0 = oracle_states_sn(size, latent)
    for k, v in eng.sn_views().items():
        v.copy_(sn0[k])
    ren = lambda k: k + "_orig" if k.endswith(".weight") else k
    row = {}

    # ---- D step ----
    met = eng.d_step(cuda(real), cuda(z), masks)
    s_d = hip_signs_d(eng, size, batch, 2)
    d_hip = {k: v.cpu().clone() for k, v in eng.views("d", "grads").items()}
    sn_hip = {k: v.cpu().clone() for k, v in eng.sn_views().items()}
    # ---- G step on the state the D step left ----
    gmet = eng.g_step(batch, cuda(z2))
    s_g = hip_signs_g(eng, size, batch) + hip_signs_d(eng, size, batch, 1)
    g_hip = {k: v.cpu().clone() for k, v in eng.views("g", "grads").items()}

    def run(signs_d, signs_g, rec_d=None, rec_g=None):
        g_sd, d_sd, g_opt, d_opt, sn = oracle_states_sn(size, latent)
        dm, dg = O.d_step(g_sd, d_sd, d_opt, real, z, masks[:nb], masks[nb:], size, signs=signs_d, record=rec_d, sn=sn)
        sn_after_d = {k: v.clone() for k, v in sn.items()}
        gm, gg = O.g_step(g_sd, d_sd, g_opt, z2, size, signs=signs_g, record=rec_g, sn=sn)
        return dm, dg, gm, gg, sn_after_d, g_sd, d_sd, g_opt, d_opt
    rec_d, rec_g = [], []
    dm, dg, gm, gg, sn_b, g_sd, d_sd, g_opt, d_opt = run(s_d, s_g, rec_d, rec_g)
    count_sign_flips(s_d, rec_d, keep=masks)
    count_sign_flips(s_g, rec_g)
    for k in DK:
        assert_close(met[k], dm[k], 2e-4, 2e-6, f"SN d metric {k} vs oracle")
        assert_close(met[k], f[f"{tag}/d/metric/{k}"], 2e-4, 2e-6, f"SN d metric {k} vs golden")
    for k in GK:
        assert_close(gmet[k], gm[k], 2e-4, 2e-6, f"SN g metric {k} vs oracle")
        assert_close(gmet[k], f[f"{tag}/g/metric/{k}"], 2e-4, 2e-6, f"SN g metric {k} vs golden")
    sc_d, _ = _scales(dg, list(dg), np.array([float(dg[k].norm()) for k in dg]))
    sc_g, _ = _scales(gg, list(gg), f[f"{tag}/g/grad_norm"])
    # (round 2 allowed 5e-3 here and blamed the cancellation in G / sigma - (<G, W> / sigma^2) u v^T; with the sign decisions
    # shared the arithmetic agrees to 1.4e-6 / 1.5e-5 -- it was the decisions all along)
    row["hip_vs_oracle_with_hip_signs_d"] = max(float((d_hip[k] - dg[k]).abs().max()) / sc_d[k] for k in dg)
    row["hip_vs_oracle_with_hip_signs_g"] = max(float((g_hip[k] - gg[k]).abs().max()) / sc_g[k] for k in gg)
    assert row["hip_vs_oracle_with_hip_signs_d"] <= 1e-4 and row["hip_vs_oracle_with_hip_signs_g"] <= 1e-4, row
    for k, v in sn_hip.items():                                # two power iterations later
        _scale_close(v.numpy(), sn_b[k].numpy(), f"SN buffer {k} vs oracle", 1e-4)
        _scale_close(probe(v, k), f[f"{tag}/d/buf/{k}"], f"SN buffer {k} vs golden", 1e-4)
    for k, v in eng.sn_views().items():                        # D.eval(): untouched by the G step
        _scale_close(probe(v.cpu(), k), f[f"{tag}/g/dbuf/{k}"], f"SN buffer {k} after the G step", 1e-5)
    i_g, i_d, i_gopt, i_dopt, _ = oracle_states_sn(size, latent)
    for which, og, oopt, sc, isd, iopt in (("d", dg, d_opt, sc_d, i_d, i_dopt), ("g", gg, g_opt, sc_g, i_g, i_gopt)):
        mv = eng.views(which, "exp_avg")
        for k in mv:
            assert float((mv[k].cpu() - oopt.m[k]).abs().max()) <= 1e-4 * sc[k], (which, k, "exp_avg")
        _weights_in_envelope(eng, which, og, sc, isd, iopt, 1e-4, oopt.step, f"SN {which}")
    # ---- the reference run's own decisions -> the fixture, on this host; HIP decisions counted against them ----
    _, cdg, _, cgg, *_ = run(census_signs(f, f"{tag}/d"), census_signs(f, f"{tag}/g"))
    row["oracle_with_reference_signs_vs_reference_d"] = max(float(np.abs(probe(cdg[k], ren(k)) - f[f"{tag}/d/grad/{ren(k)}"]).max()) / sc_d[k] for k in cdg)
    row["oracle_with_reference_signs_vs_reference_g"] = _golden_rel(f, f"{tag}/g", cgg, list(cgg), sc_g)
    assert row["oracle_with_reference_signs_vs_reference_d"] <= 1e-4 and row["oracle_with_reference_signs_vs_reference_g"] <= 1e-4, row
    fl_d = flips_vs_census(f, f"{tag}/d", s_d, keep=masks)
    fl_g = flips_vs_census(f, f"{tag}/g", s_g)
    row["flips_vs_reference_d"], row["flips_vs_reference_g"] = len(fl_d), len(fl_g)
    hip_d = max(float(np.abs(probe(d_hip[k], ren(k)) - f[f"{tag}/d/grad/{ren(k)}"]).max()) / sc_d[k] for k in d_hip)
    prd_d = max(float(np.abs(probe(dg[k], ren(k)) - f[f"{tag}/d/grad/{ren(k)}"]).max()) / sc_d[k] for k in dg)
    hip_g, prd_g = _golden_rel(f, f"{tag}/g", g_hip, list(gg), sc_g), _golden_rel(f, f"{tag}/g", gg, list(gg), sc_g)
    row.update(hip_vs_reference_d=hip_d, hip_vs_reference_g=hip_g, predicted_by_the_flips_d=prd_d, predicted_by_the_flips_g=prd_g)
    assert (hip_d <= 1e-3) if not fl_d else (abs(hip_d - prd_d) <= 1e-3), row
    assert (hip_g <= 1e-3) if not (fl_d or fl_g) else (abs(hip_g - prd_g) <= 1e-3), row
    MARGINS[f"spectral_norm/{tag}"] = row
    _dump_margins()
    eng.close()


@pytest.mark.parametrize("size,latent,batch", [(64, 100, 8), (128, 128, 4)])
def test_spectral_norm_pipelined_step_equals_split_steps(size, latent, batch):
    """siggan_step_begin with a spectral-norm Discriminator (what VanillaGAN(use_spectral_norm=True).train_step, GANTrainer,
    Engine.train_step and DataParallelStep.step call): the SN D phase has no pipelined Generator forward, so siggan_g_grads
    must run the training forward itself on the z handed to step_begin.  Same inputs -> the same bits as d_step + g_step
    (which test_spectral_norm_training holds to the reference's own fixture): parameters, Adam moments, BatchNorm buffers
    (the running statistics MUST move), u / v and every metric."""
    from hipcommon import cuda, load_engine_state
    from signature_gan_amd.engine import Engine
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, d_chans(size) * 2, 9)]
    z = cuda(torch.from_numpy(I.gen_z(batch, latent, SEED["z"])))
    z2 = cuda(torch.from_numpy(I.gen_z(batch, latent, SEED["z"] + 1)))
    real = cuda(torch.from_numpy(I.gen_real(batch, size, SEED["real"])))
    _, _, _, _, sn = oracle_states_sn(size, latent)

    def engine():
        e = load_engine_state(Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", spectral_norm=True),
                              size, latent, warm=True)
        for k, v in e.sn_views().items():
            v.copy_(sn[k])
        return e

    def state(e):
        return [t.clone() for t in (e.g_params, e.d_params, e.g_exp_avg, e.g_exp_avg_sq, e.d_exp_avg, e.d_exp_avg_sq, e.g_bn_mean,
                                    e.g_bn_var, e.g_bn_batches, e.g_adam_steps, e.d_adam_steps, e.d_sn_u, e.d_sn_v)]

    a = engine()
    bn0 = a.g_bn_mean.clone()
    ref_m = []
    for s in range(2):
        m = a.d_step(real, z, masks, clip=0.5)
        m.update(a.g_step(batch, z2, clip=0.5))
        ref_m.append(m)
    ref = state(a)
    assert not torch.equal(bn0, a.g_bn_mean), "the G step's training forward did not move the running statistics"
    a.close()
    for explicit_zg in (True, False):
        b = engine()
        got_m = []
        for s in range(2):
            if explicit_zg:
                got_m.append(b.train_step(real, z, masks, z2, clip=0.5))
            else:               # the same step cut as DataParallelStep.step cuts it, z_g handed to g_grads instead
                b.step_begin(real, z, masks, None)
                m = b.d_apply(clip=0.5)
                b.g_compute_grads(batch, z2)
                m.update(b.g_apply(clip=0.5))
                got_m.append(m)
        assert got_m == ref_m, (explicit_zg, got_m, ref_m)
        for x, y in zip(ref, state(b)):
            assert torch.equal(x, y), f"pipelined SN step (explicit z_g: {explicit_zg}) differs from d_step + g_step"
        b.close()


def test_spectral_norm_drop_in_modules():
    """VanillaGAN(use_spectral_norm=True): the reference's SN keys as views of the engine's storage; a train_step moves
    weight_orig, weight_u and weight_v; eval-mode scoring leaves the buffers alone; the ablation step variant runs with it."""
    from signature_gan_amd.vanilla_gan_model import VanillaGAN
    m = VanillaGAN(latent_dim=100, image_size=64, device="cuda:0", max_batch=8, use_spectral_norm=True, seed=5)
    sd = m.discriminator.state_dict()
    assert [k for k in sd if k.startswith("conv_blocks.0")] == ["conv_blocks.0.block.0.bias", "conv_blocks.0.block.0.weight_orig",
                                                               "conv_blocks.0.block.0.weight_u", "conv_blocks.0.block.0.weight_v"]
    before = {k: v.clone() for k, v in sd.items()}
    real = torch.rand(8, 1, 64, 64, device="cuda:0") * 2 - 1
    met = m.train_step(real)
    assert np.isfinite(met["d_loss"]) and np.isfinite(met["g_loss"])
    after = m.discriminator.state_dict()
    for k in ("classifier.0.weight_orig", "classifier.0.weight_v", "conv_blocks.2.block.0.weight_u"):
        assert not torch.equal(before[k], after[k]), k
    for k in ("classifier.0.weight_u", "classifier.0.weight_v", "conv_blocks.3.block.0.weight_u"):
        assert abs(float(after[k].norm()) - 1.0) < 1e-4, k
    snap = {k: v.clone() for k, v in after.items()}
    m.discriminator.eval()
    p = m.discriminator(real)
    assert p.shape == (8, 1) and bool(((p > 0) & (p < 1)).all())
    for k, v in m.discriminator.state_dict().items():
        assert torch.equal(v, snap[k]), k
    m.engine.set_step_variant("ablation")
    am = m.engine.ablation_step(real)
    assert np.isfinite(am["d_loss"]) and np.isfinite(am["g_loss"])
