"""The sigmoid / BCE heads at saturated predictions, in every path that holds a copy of them: bce_block, bce_dlogit and
k_cls_bwd_eval (ops.hip) and the verifier trainer's head (verifier_train.hip), against the reference's fp32 head restated in
headcommon.py (pinned to torch on the CPU by test_saturated_heads_cpu.py).

A Discriminator that wins drives D(G(z)) to exactly 0, a collapsing one to exactly 1, and the reference's fp32 arithmetic is
sharp there: p == 1 from x = 24 ln 2 (loss 100 (1 - y), gradient 0), the 1e-12 floor under (1 - p) p from x = -27.63 (the
gradient decays like p), a subnormal p at -88 whose log is still -88, p == 0 below -88.72 (loss 100 y).  Every other test of
the project keeps |logit| < 12.

Bounds (none of them is a measured figure):
  p        2 ulp of headcommon.p_ref: expf good to 1 ulp, one rounded add, one correctly rounded divide.
  d(logit) 8 ulp of dlogit_ref evaluated from the DEVICE's fp32 p: five roundings (p - y, (1 - p) p, the divide, times
           1 / count, the final product), doubled.  An ulp is the fp32 spacing at the reference value, i.e. 2^-149 for a
           subnormal one; a reference of exactly 0 requires +-0; a reference below 2^-126 may also come out as 0 -- a
           flushed subnormal gradient has no consequence (Adam's eps is 1e-8, the fp16 chains scale by 1024 first).
  losses and means of p   8 ulp of the fp64 mean of loss_ref(device p, y) resp. of p.
  accuracies              the exact counts of p > 0.5 / p < 0.5 over the segment (times the fp32 1 / B: one rounding).
  classifier weight gradient   (N + 2) 2^-24 sum_n |d(logit)_n act_n| per element, N the rows the sum runs over (an fma chain of
           N terms and the two adds of k_cls_wgrad's four row lanes); the bias gradient the same with act = 1.
Admissibility (headcommon.regime) is asserted on the device's logits: the inputs are chosen so that it holds."""
import numpy as np
import pytest
import torch

import headcommon as H
from common import I, O, SEED

pytestmark = pytest.mark.gpu
SIZE, LATENT = 64, 100
ULP_P, ULP = 2, 8
TINY = 2.0 ** -126
# worst observed fraction of each bound, per case: the hook profiles/saturated_heads_margins.py reads and writes out
MARGINS = {}


def _note(row, key, frac):
    row[key] = max(row.get(key, 0.0), float(frac))


def _inputs(batch, passes):
    from hipcommon import cuda
    z = cuda(torch.from_numpy(I.gen_z(batch, LATENT, SEED["z"])))
    z2 = cuda(torch.from_numpy(I.gen_z(batch, LATENT, SEED["z"] + 1)))
    real = cuda(torch.from_numpy(I.gen_real(batch, SIZE, SEED["real"])))
    masks = [torch.from_numpy(m) for m in I.gen_masks(batch, list(O.D_CHAIN[SIZE]) * passes, 5)]
    return z, z2, real, masks


def _gscale(eng):
    """What the backward chains of a context carry on top of the gradient: the fp16 static scale (default 1024), else 1."""
    return (eng.f16_grad_scale or 1024.0) if eng.dtype == "f16" else 1.0


# ---- the per-row checks every head shares ---------------------------------------------------------------------------
def check_p(logits, p, row, what):
    """Device p (float32 array) of device logits: admissible, finite, within 2 ulp of p_ref, exact at the ends and at 0."""
    assert logits.dtype == np.float32 and p.dtype == np.float32
    for x in logits:
        assert H.regime(x, 0).admissible, f"{what}: logit {x!r} is within {H.MARGIN} of a decision point: the case is mis-set"
    assert np.isfinite(p).all(), f"{what}: p {p}"
    d = H.ulp_distance32(p, H.p_ref(logits))
    assert d.max() <= ULP_P, f"{what}: p {p} vs {H.p_ref(logits)} ({d.max()} ulp)"
    _note(row, "p", d.max() / ULP_P)
    assert (p[logits > H.X_ONE] == 1.0).all() and (p[logits < H.X_ZERO] == 0.0).all() and (p[logits == 0.0] == 0.5).all(), f"{what}: p {p}"
    assert (p[(logits > H.X_ZERO) & (logits < H.X_ONE)] > 0.0).all(), f"{what}: a subnormal p was flushed: {p}"


def check_dlogit(p, dl, ys, count, row, what):
    """Device d(logit) (fp64 array, any gradient scale already divided out) against dlogit_ref(device p)."""
    assert np.isfinite(dl).all(), f"{what}: d(logit) {dl}"
    ref = H.dlogit_ref(p, ys, count)                       # ys: one target, or one per row
    u = H.ulps(dl, ref)
    ok = np.where(ref == 0.0, dl == 0.0, (u <= ULP) | ((np.abs(ref) < TINY) & (dl == 0.0)))
    assert ok.all(), f"{what}: d(logit) {dl} vs {ref} ({u} ulp)"
    live = (ref != 0.0) & (dl != 0.0)
    _note(row, "dlogit", u[live].max() / ULP if live.any() else 0.0)
    return ref


def check_mean(got, vals64, row, key, what):
    """A metric (fp32 scalar) against the fp64 mean of per-row fp64 values: 8 ulp; a mean of exactly 0 requires +-0."""
    want = float(np.mean(vals64))
    assert np.isfinite(got), f"{what}: {got}"
    if want == 0.0:
        assert got == 0.0, f"{what}: {got!r}, the reference is exactly 0"
        return
    u = float(H.ulps(got, want))
    assert u <= ULP, f"{what}: {got!r} vs {want!r} ({u:.2f} ulp)"
    _note(row, key, u / ULP)


def check_acc(got, p, above, what):
    n = int((p > 0.5).sum()) if above else int((p < 0.5).sum())
    if n == 0:
        assert got == 0.0, f"{what}: {got!r} with no such prediction"
    else:
        assert abs(got - n / p.size) <= 2.0 ** -23 and round(got * p.size) == n, f"{what}: {got!r}, {n} of {p.size}"


def _metrics(eng):
    from signature_gan_amd import _lib
    m = eng.metrics.cpu().numpy()
    return {k: m[i] for k, i in _lib.METRIC_INDEX.items()}


# ---- 2. head level: zero classifier weight, bias = x0 --------------------------------------------------------------
# launch_gconv's split rule (gconv.hip) decides the form the step's logits are left in (LogitSrc): the last Discriminator block
# at 64x64 is a down GEMM of M = 16 B rows, Co = 512, nk = 16 * 256 / 32 = 128 K-tiles.  Its 64x64 tiling gives
# nblk = ceil(B / 4) * 8 workgroups; splits() asks for ns = min(ceil(512 / nblk), nk / 4, 8) slabs while nblk < 384, and the
# classifier's dot product rides in the split-K epilogue (launch_cfg: a.cls_w survives, 8 partials per image, LogitSrc::P = 8)
# exactly when ns > 2 slabs run through k_splitk_epilogue: ns == 2 is ONE launch of 8-wave workgroups with nsplit == 1 and
# no epilogue kernel, ns == 1 has none either, and launch_cfg then drops cls_w -- k_cls_fwd stores the logits (P = 0).
# ns <= 2 first holds at nblk >= 256, i.e. ceil(B / 4) = 32: batch 125 is the smallest batch with STORED logits, every batch
# below it (5 here: odd segment counts, a ragged row tile) leaves split-K PARTIALS.  Established from the rule as read in the
# code: both forms run the same kernel slot (k_gconv<64,64>), so the launch profile does not tell them apart.
BATCH_PARTIALS, BATCH_STORED = 5, 125


def _head_rows(eng, x0, r0, n, ys, count, row, what):
    lg = eng.debug_tensor("logits", 0, (r0 + n,)).cpu().numpy()[r0:]
    p = eng.debug_tensor("probs", 0, (r0 + n,)).cpu().numpy()[r0:]
    dl_raw = eng.debug_tensor("dlogit", 0, (r0 + n,)).cpu().numpy()[r0:].astype(np.float64)
    assert (lg == np.float32(x0)).all(), f"{what}: logits {lg} are not the bias {x0} (zero weight)"
    check_p(lg, p, row, what)
    check_dlogit(p, dl_raw / _gscale(eng), ys, count, row, what)
    return p, dl_raw


@pytest.mark.parametrize("batch", [BATCH_PARTIALS, BATCH_STORED])
@pytest.mark.parametrize("variant", ["trainer", "ablation"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_head_sweep_in_the_step(dtype, variant, batch):
    """classifier.0.weight = 0, classifier.0.bias = x0: every image of a D phase and of a G phase has logit x0, for every x0
    of the sweep.  bce_block (metrics, p, d(logit)) and k_cls_wgrad on what it wrote; bce_dlogit inside k_cls_bwd is held by the
    exactly-zero arenas here and by the chain tests below.  Batch 5: split-K partials; 125: stored logits (see above).  The
    G phase's rows start at B in the trainer variant and at 0 in the ablation variant (whose G target is the smoothed 0.9)."""
    from hipcommon import make_engine
    B, abl = batch, variant == "ablation"
    eng = make_engine(SIZE, LATENT, B, warm=True, dtype=dtype)
    if abl:
        eng.set_step_variant("ablation")
    gs = _gscale(eng)
    z, z2, real, masks = _inputs(B, 3 if abl else 2)
    dv, Ld, C = eng.views("d"), len(O.D_CHAIN[SIZE]), O.D_CHAIN[SIZE][-1]
    row = MARGINS.setdefault(f"sweep/{dtype}/{variant}/b{B}", {})
    ys_d = np.array([0.9] * B + [0.0] * B)
    gy = 0.9 if abl else 1.0
    for x0 in H.X0:
        what = f"{dtype} {variant} b{B} x0={x0}"
        dv["classifier.0.weight"].zero_(); dv["classifier.0.bias"].fill_(x0)
        eng.params_changed()
        eng.d_grads.fill_(7.0); eng.g_grads.fill_(7.0)          # every gradient below was written by this pass
        # ---- D phase: rows [0, B) real against 0.9, [B, 2B) fake against 0 ----
        eng.d_compute_grads(real, z, masks, 0.9, mask_passes=3 if abl else 2)
        p, dl = _head_rows(eng, x0, 0, 2 * B, ys_d, B, row, what + " D")
        m = _metrics(eng)
        pr, pf = p[:B], p[B:]
        lr, lf = H.loss_ref(pr, 0.9), H.loss_ref(pf, 0.0)
        check_mean(m["d_loss_real"], lr, row, "d_loss_real", what + " d_loss_real")
        check_mean(m["d_loss_fake"], lf, row, "d_loss_fake", what + " d_loss_fake")
        check_mean(m["d_loss"], [np.mean(lr) + np.mean(lf)], row, "d_loss", what + " d_loss")
        check_mean(m["d_real_mean"], pr.astype(np.float64), row, "d_real_mean", what + " d_real_mean")
        check_mean(m["d_fake_mean"], pf.astype(np.float64), row, "d_fake_mean", what + " d_fake_mean")
        check_acc(m["d_real_acc"], pr, True, what + " d_real_acc")
        check_acc(m["d_fake_acc"], pf, False, what + " d_fake_acc")
        if x0 == -88.0:                                         # the reference keeps the subnormal p: 0.9 * 88, not 0.9 * 100
            assert abs(float(m["d_loss_real"]) - 0.9 * 88.0) < 1e-4, m["d_loss_real"]
        grads = {k: v.cpu().numpy().astype(np.float64) / gs for k, v in eng.views("d", "grads").items()}
        act = eng.debug_tensor("d_a", Ld, (2 * B, 16, C)).cpu().numpy().astype(np.float64)     # (n, hw, c)
        d = dl / gs
        want_w = np.einsum("n,nhc->ch", d, act).reshape(-1)     # the reference's c, h, w order
        bound_w = (2 * B + 2) * 2.0 ** -24 * np.einsum("n,nhc->ch", np.abs(d), np.abs(act)).reshape(-1)
        got_w = grads["classifier.0.weight"].reshape(-1)
        assert np.isfinite(got_w).all() and (np.abs(got_w - want_w) <= bound_w).all(), \
            f"{what}: classifier weight gradient off by {np.abs(got_w - want_w).max():.3e}"
        if bound_w.max() > 0:
            _note(row, "cls_weight_grad", (np.abs(got_w - want_w)[bound_w > 0] / bound_w[bound_w > 0]).max())
        got_b, bound_b = float(grads["classifier.0.bias"][0]), (2 * B + 2) * 2.0 ** -24 * np.abs(d).sum()
        assert abs(got_b - d.sum()) <= bound_b, f"{what}: classifier bias gradient {got_b!r} vs {d.sum()!r}"
        if bound_b > 0:
            _note(row, "cls_bias_grad", abs(got_b - d.sum()) / bound_b)
        for k, g in grads.items():
            if not k.startswith("classifier."):
                assert (g == 0.0).all(), f"{what}: D gradient {k} is not exactly zero behind a zero classifier weight"
        # ---- G phase ----
        eng.g_compute_grads(B, None if abl else z2, label_smoothing=0.9)
        r0 = 0 if abl else B
        p, _ = _head_rows(eng, x0, r0, B, gy, B, row, what + " G")
        m = _metrics(eng)
        check_mean(m["g_loss"], H.loss_ref(p, gy), row, "g_loss", what + " g_loss")
        check_mean(m["g_fake_mean"], p.astype(np.float64), row, "g_fake_mean", what + " g_fake_mean")
        if x0 == -88.0:
            assert abs(float(m["g_loss"]) - gy * 88.0) < 1e-4, m["g_loss"]
        assert bool((eng.g_grads == 0.0).all()), f"{what}: a Generator gradient is not exactly zero behind a zero classifier weight"
    eng.close()


# ---- 3. through the whole chain: the classifier's weight restored, only its bias shifted -------------------------------
LOGIT_SPREAD = (-4.3, 4.0)         # 64x64, batch <= 16, warm test state: every logit of the existing step cases (oracle, CPU)


def _sn_engine(B):
    from common import oracle_states_sn
    from hipcommon import load_engine_state
    from signature_gan_amd.engine import Engine
    eng = load_engine_state(Engine(latent_dim=LATENT, image_size=SIZE, max_batch=B, device="cuda:0", spectral_norm=True),
                            SIZE, LATENT, warm=True)
    _, _, _, _, sn0 = oracle_states_sn(SIZE, LATENT)
    for k, v in eng.sn_views().items():
        v.copy_(sn0[k])
    return eng


def _engine(kind, B):
    from hipcommon import make_engine
    return _sn_engine(B) if kind == "sn" else make_engine(SIZE, LATENT, B, warm=True, dtype=kind)


def _shift(eng, b):
    eng.views("d")["classifier.0.bias"].add_(b)
    eng.params_changed()


def _logits_in_range(eng, b, r0, n, what):
    lg = eng.debug_tensor("logits", 0, (r0 + n,)).cpu().numpy()[r0:]
    assert np.isfinite(lg).all() and lg.min() >= b + LOGIT_SPREAD[0] and lg.max() <= b + LOGIT_SPREAD[1], f"{what}: logits {lg}"
    for x in lg:
        assert H.regime(x, 0).admissible, f"{what}: logit {x!r}"
    return lg


def _adam_zero_grad(eng, which, before, what):
    """Parameters and both moments after an update with an all-zero gradient: O.adam_update from the warm moments, within
    test_ops_gpu.test_adam's bounds (moments 1e-5 of their scale, parameters 2e-7 + 1e-6 * lr)."""
    step = int(before["step"]) + 1
    p, m, v = before["p"].clone(), before["m"].clone(), before["v"].clone()
    O.adam_update(p, torch.zeros_like(p), m, v, step, 2e-4, 0.5, 0.999)
    for name, want, got in (("exp_avg", m, getattr(eng, f"{which}_exp_avg")), ("exp_avg_sq", v, getattr(eng, f"{which}_exp_avg_sq"))):
        got = got.cpu()
        assert torch.isfinite(got).all()
        assert float((got.double() - want.double()).abs().max()) <= 1e-5 * float(want.abs().max()), f"{what}: {name}"
    got = getattr(eng, f"{which}_params").cpu()
    assert torch.isfinite(got).all()
    assert float((got - p).abs().max()) <= 2e-7 + 1e-6 * 2e-4, f"{what}: parameters"
    assert float(getattr(eng, f"{which}_adam_steps")[0]) == step


def _snapshot(eng, which):
    return {"p": getattr(eng, f"{which}_params").cpu().clone(), "m": getattr(eng, f"{which}_exp_avg").cpu().clone(),
            "v": getattr(eng, f"{which}_exp_avg_sq").cpu().clone(), "step": float(getattr(eng, f"{which}_adam_steps")[0])}


_BN_UNSHIFTED = {}


def _bn_after_unshifted_g_step(kind, B, z2):
    """BatchNorm running statistics after one G step of the UNSHIFTED warm state (the forward does not depend on the bias)."""
    if kind not in _BN_UNSHIFTED:
        eng = _engine(kind, B)
        eng.g_step(B, z2, clip=0.5)
        _BN_UNSHIFTED[kind] = {k: v.cpu().clone() for k, v in eng.bn_views().items()}
        eng.close()
    return _BN_UNSHIFTED[kind]


@pytest.mark.parametrize("b", [-95.0, 25.0])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16", "sn"])
def test_dead_regimes_through_the_chain(kind, b):
    """Every p exactly 0 (bias - 95) or exactly 1 (bias + 25) with the trained classifier weight in place: one D step and one
    G step with clip = 0.5.  bce_dlogit inside k_cls_bwd must hand the chain exact zeros -- 0 / 1e-12 * 0, never 0 * inf."""
    B = 5
    eng = _engine(kind, B)
    z, z2, real, masks = _inputs(B, 2)
    bn_want = _bn_after_unshifted_g_step(kind, B, z2)
    _shift(eng, b)
    what = f"{kind} b={b}"
    row = MARGINS.setdefault(f"dead/{kind}/{b:+.0f}", {})
    # ---- D step ----
    before = _snapshot(eng, "d")
    eng.d_grads.fill_(7.0)
    m = eng.d_step(real, z, masks, clip=0.5)
    _logits_in_range(eng, b, 0, 2 * B, what + " D")
    p = eng.debug_tensor("probs", 0, (2 * B,)).cpu().numpy()
    assert (p == (0.0 if b < 0 else 1.0)).all(), p
    assert bool((eng.d_grads == 0.0).all()), f"{what}: the D gradient arena is not exactly zero"
    assert m["d_grad_norm"] == 0.0 and _metrics(eng)["d_skipped"] == 0.0
    assert all(np.isfinite(v) for v in m.values())
    if b < 0:
        assert (m["d_loss_real"], m["d_loss_fake"], m["d_loss"]) == (90.0, 0.0, 90.0), m
        assert (m["d_real_mean"], m["d_fake_mean"], m["d_real_acc"], m["d_fake_acc"]) == (0.0, 0.0, 0.0, 1.0), m
    else:
        want = 100.0 * (1.0 - float(np.float32(0.9)))                  # 10.000002
        u = float(H.ulps(m["d_loss_real"], want))
        assert u <= ULP, (m["d_loss_real"], want)
        _note(row, "d_loss_real", u / ULP)
        assert m["d_loss_fake"] == 100.0 and float(H.ulps(m["d_loss"], want + 100.0)) <= ULP, m
        assert (m["d_real_mean"], m["d_fake_mean"], m["d_real_acc"], m["d_fake_acc"]) == (1.0, 1.0, 1.0, 0.0), m
    _adam_zero_grad(eng, "d", before, what + " D")
    # ---- G step (the D update with a zero gradient moved the weights by the warm moments: the range still holds) ----
    before = _snapshot(eng, "g")
    eng.g_grads.fill_(7.0)
    m = eng.g_step(B, z2, clip=0.5)
    r0 = 0 if kind == "sn" else B
    lg = eng.debug_tensor("logits", 0, (r0 + B,)).cpu().numpy()[r0:]
    assert np.isfinite(lg).all() and (lg < H.X_ZERO - H.MARGIN if b < 0 else lg > H.X_ONE + H.MARGIN).all(), lg
    p = eng.debug_tensor("probs", 0, (r0 + B,)).cpu().numpy()[r0:]
    assert (p == (0.0 if b < 0 else 1.0)).all(), p
    assert bool((eng.g_grads == 0.0).all()), f"{what}: the G gradient arena is not exactly zero"
    assert m["g_grad_norm"] == 0.0 and _metrics(eng)["g_skipped"] == 0.0
    assert (m["g_loss"], m["g_fake_mean"]) == ((100.0, 0.0) if b < 0 else (0.0, 1.0)), m
    _adam_zero_grad(eng, "g", before, what + " G")
    for k, v in eng.bn_views().items():
        assert torch.equal(v.cpu(), bn_want[k]), f"{what}: BatchNorm buffer {k} moved differently from the unshifted run"
    eng.close()


@pytest.mark.parametrize("b", [-60.0, -35.0, -27.0, 10.0])
def test_live_regimes_through_the_chain(b):
    """The floor regime (-60, -35), its edge (-27) and the coarse 1 - p side (+10) with the trained classifier weight, f32,
    batch 5: one D step, then one G step on the state it left, against O.d_step / O.g_step (torch's own fp32 sigmoid / BCE on
    the CPU) on the same shifted state, handed the HIP path's sign decisions as test_engine_gpu.test_single_steps does.
    Gradients: 1e-4 of each tensor's scale (hipcommon.grad_scales); metrics: assert_close(2e-4, 2e-6).  The G step is left out
    at +10: there 1 - p is a handful of fp32 quanta and one quantum of p is several percent of the gradient, in the
    reference as well."""
    from common import assert_close, oracle_states
    from hipcommon import count_sign_flips, grad_scales, hip_signs_d, hip_signs_g, make_engine
    B = 5
    eng = make_engine(SIZE, LATENT, B, warm=True)
    _shift(eng, b)
    g_sd, d_sd, g_opt, d_opt = oracle_states(SIZE, LATENT, warm=True)
    d_sd["classifier.0.bias"] += b
    z, z2, real, masks = _inputs(B, 2)
    nb = len(masks) // 2
    row = MARGINS.setdefault(f"live/f32/{b:+.0f}", {})

    def grads_close(which, o_grads, what):
        gv = eng.views(which, "grads")
        scale = grad_scales(o_grads, list(gv))
        for k, t in gv.items():
            assert torch.isfinite(t).all(), f"{what} grad {k}"
            err = float((t.cpu() - o_grads[k]).abs().max()) / scale[k]
            _note(row, f"{which}_grads", err / 1e-4)
            assert err <= 1e-4, f"{what} grad {k}: {err:.3e} of scale {scale[k]:.3e}"

    met = eng.d_step(real, z, masks)
    _logits_in_range(eng, b, 0, 2 * B, f"b={b} D")
    signs, rec = hip_signs_d(eng, SIZE, B, 2), []
    o_met, o_grads = O.d_step(g_sd, d_sd, d_opt, real.cpu(), z.cpu(), masks[:nb], masks[nb:], SIZE, signs=signs, record=rec)
    count_sign_flips(signs, rec, keep=masks)
    for k in ("d_loss", "d_loss_real", "d_loss_fake", "d_real_mean", "d_fake_mean"):
        assert_close(met[k], o_met[k], 2e-4, 2e-6, f"b={b} {k}")
    grads_close("d", o_grads, f"b={b} D")
    if b < 0:
        met = eng.g_step(B, z2)
        lg = eng.debug_tensor("logits", 0, (2 * B,)).cpu().numpy()[B:]
        assert np.isfinite(lg).all() and all(H.regime(x, 1).admissible for x in lg), lg
        signs, rec = hip_signs_g(eng, SIZE, B) + hip_signs_d(eng, SIZE, B, 1), []
        o_met, o_grads = O.g_step(g_sd, d_sd, g_opt, z2.cpu(), SIZE, signs=signs, record=rec)
        count_sign_flips(signs, rec)
        for k in ("g_loss", "g_fake_mean"):
            assert_close(met[k], o_met[k], 2e-4, 2e-6, f"b={b} {k}")
        grads_close("g", o_grads, f"b={b} G")
    eng.close()


# ---- 4. the latent objective's classifier tail (k_cls_bwd_eval) ------------------------------------------------------
@pytest.mark.parametrize("sn", [False, True], ids=["plain", "sn"])
def test_latent_objective_at_saturated_scores(sn):
    """siggan_g_latent_objective_grad with the Discriminator's bias shifted by -95 (every p == 0), -35 (the floor regime) and
    +25 (every p == 1) on test_latent_objective_gpu's state (|logit| < 6 unshifted), B = 5, weights (0, 1, 0) and (1, 1, 0.1).
    At -35 the yardstick is objectivecommon's fp64 oracle on the device's decisions with the reference's fp32 head in place of
    the mathematical one: dz_ref = w_r dz_recon + w_d dlogit_ref(device p) dlogit/dz + w_p dz_prior, where dlogit/dz is the
    oracle's realism gradient divided by its own d softplus(-x) / dx = -sigmoid(-x) (1 to 1e-15 there); that test's bound,
    1e-4 of max|dz_ref|."""
    from hipcommon import hip_signs_g
    from latentcommon import oracle_sd64
    from objectivecommon import GAIN, hip_signs_d_rows, lut_f32, objective_engine, oracle_d_sd64, oracle_objective
    B = 5
    eng = objective_engine(SIZE, LATENT, B, 0.0, sn)
    z = torch.from_numpy(I.gen_z(B, LATENT, SEED["z"]))
    zc = z.cuda()
    t_u8 = eng.g_generate_u8(torch.from_numpy(I.gen_z(B, LATENT, SEED["z"] + 1)).cuda())
    uv = {k: v.cpu().clone() for k, v in eng.sn_views().items()} if sn else None
    bias = eng.views("d")["classifier.0.bias"]
    bias0 = bias.clone()
    row = MARGINS.setdefault(f"latent_objective/{'sn' if sn else 'plain'}", {})
    W1, W3, W3_NO_D = (0.0, 1.0, 0.0), (1.0, 1.0, 0.1), (1.0, 0.0, 0.1)
    f32 = np.float32
    for b in (-95.0, -35.0, 25.0):
        what = f"latent objective {'sn ' if sn else ''}b={b}"
        bias.copy_(bias0 + b)
        eng.params_changed()
        dz1, obj1, terms1, p1, img1 = (t.cpu() for t in eng.g_latent_objective_grad(zc, None, *W1, want_terms=True, want_probs=True, want_images=True))
        dz3, obj3, terms3, p3, img3 = (t.cpu() for t in eng.g_latent_objective_grad(zc, t_u8, *W3, want_terms=True, want_probs=True, want_images=True))
        lg = eng.debug_tensor("logits", 0, (B,)).cpu().numpy()
        if b == -35.0:
            signs_g, signs_d = hip_signs_g(eng, SIZE, B), hip_signs_d_rows(eng, SIZE, B)
            floor = {"dz1": dz1, "dz3": dz3, "p": p3.numpy(), "logits": lg}
        dz0, obj0, terms0, _ = (t.cpu() for t in eng.g_latent_objective_grad(zc, t_u8, *W3_NO_D, want_terms=True, want_images=True))
        fwd = eng.d_forward(img3.cuda(), training=False).cpu().reshape(-1)
        assert np.isfinite(lg).all() and lg.min() >= b - 6.0 and lg.max() <= b + 6.0 and all(H.regime(x, 1).admissible for x in lg), lg
        assert torch.equal(p1, fwd) and torch.equal(p3, fwd), f"{what}: probs are not siggan_d_forward's bits"
        for t in (dz1, obj1, terms1, dz3, obj3, terms3):
            assert torch.isfinite(t).all(), what
        p = p3.numpy()
        check_p(lg, p, row, what)
        want_term = H.loss_ref(p, 1.0)
        for terms in (terms1, terms3):
            got = terms[1].numpy()
            if b == -35.0:
                u = H.ulps(got, want_term)
                assert u.max() <= ULP, f"{what}: realism term {got} vs {want_term}"
                _note(row, "realism_term", u.max() / ULP)
            else:
                assert (got == (100.0 if b < 0 else 0.0)).all() and (want_term == (100.0 if b < 0 else 0.0)).all(), f"{what}: realism term {got}"
        assert torch.equal(terms3[0], terms0[0]) and torch.equal(terms3[2], terms0[2])
        if b != -35.0:
            assert (p == (0.0 if b < 0 else 1.0)).all(), p
            assert bool((dz1 == 0.0).all()), f"{what}: the realism gradient of a dead head is not exactly zero"
            assert torch.equal(dz3, dz0), f"{what}: dz differs from the objective without the realism term"
            # latent.hip: obj = w_r recon; obj += w_d realism; obj += w_p prior -- each product and sum rounded to fp32
            rec_, real_, pri_ = (terms3[i].numpy() for i in range(3))
            want_obj = ((f32(W3[0]) * rec_).astype(f32) + (f32(W3[1]) * real_).astype(f32)).astype(f32)
            want_obj = (want_obj + (f32(W3[2]) * pri_).astype(f32)).astype(f32)
            assert np.array_equal(obj3.numpy(), want_obj), f"{what}: objective {obj3.numpy()} vs {want_obj}"
            if b > 0:
                assert torch.equal(obj3, obj0), f"{what}: a realism term of 0 changed the objective's bits"
            assert np.array_equal(obj1.numpy(), real_)
    eng.close()
    # ---- -35: the floor regime against the fp64 oracle with the reference's head ----
    d64 = dict(oracle_d_sd64(SIZE, uv))
    d64["classifier.0.bias"] = d64["classifier.0.bias"] - 35.0
    _, grads, logit_ref = oracle_objective(oracle_sd64(SIZE, LATENT, GAIN[SIZE]), d64, z, lut_f32(t_u8)[:, 0].double(), SIZE,
                                           signs_g, signs_d, 0.0)
    assert float((logit_ref - torch.from_numpy(floor["logits"]).double()).abs().max()) <= 1e-3, (logit_ref, floor["logits"])
    jac = grads[1] / (-torch.sigmoid(-logit_ref))[:, None]                    # d(logit) / dz
    dl = torch.from_numpy(H.dlogit_ref(floor["p"], 1.0, 1))[:, None]
    for w, dz in ((W1, floor["dz1"]), (W3, floor["dz3"])):
        ref = w[0] * grads[0] + w[1] * dl * jac + w[2] * grads[2]
        err = float((dz.double() - ref).abs().max()) / float(ref.abs().max())
        _note(row, f"dz_floor_regime{w}", err / 1e-4)
        assert float(ref.abs().max()) > 0 and err <= 1e-4, f"latent objective b=-35 {w}: {err:.3e} of max|dz_ref| {float(ref.abs().max()):.3e}"


# ---- 5. the verifier trainer's head (verifier_train.hip) and the inference path's score (verifier.hip) --------------------
V_PAIRS, V_E = 3, 40
V_X0 = (-95.0, -30.0, 0.0, 16.7, 30.0)
_V_REF = {}


def _verifier_encoder_reference(dec):
    """TC.train_grads (contrastive on) in fp64 and on the same fp32 state, classifier.3.weight = 0, given HIP's decisions:
    with a zero weight nothing reaches the encoder through the head, whatever its bias, so one pair of runs serves every x0."""
    import verifiertraincommon as TC
    key = tuple(bytes(np.asarray(dec[k]).tobytes()) for k in sorted(dec))
    if key not in _V_REF:
        out = []
        for dt in (torch.float64, torch.float32):
            P, R = TC.state(V_E, dt)
            P["classifier.3.weight"].zero_()
            out.append(TC.train_grads(P, R, TC.case_batch(V_PAIRS, dt), True, decisions=dec)["grads"])
        _V_REF.clear()
        _V_REF[key] = out
    return _V_REF[key]


@pytest.mark.parametrize("use_c", [True, False], ids=["contrastive", "bce_only"])
def test_verifier_head_sweep(use_c):
    """classifier.3.weight = 0, classifier.3.bias = x0: every pair's logit is x0 (labels 1, 0, 1; explicit masks; E = 40).  The
    trainer exposes the similarity per pair and the batch's BCE, so the BCE is held to the fp64 mean of loss_ref(device p,
    label) and d(logit) through the bias gradient: sum_i dlogit_ref(device p_i, y_i, B) within 8 ulp per pair plus the
    (B + 2) 2^-24 of the sum.  Encoder gradients (contrastive on): the bound test_big_batch_against_the_restatement forms,
    min(32 x the fp32 restatement's own deviation from fp64, 1e-4) of each tensor's max-abs."""
    import test_verifier_train_gpu as VT
    import verifiertraincommon as TC
    from verifiertraincommon import TI, VC
    import signature_gan_amd  # noqa: F401
    from signature_gan_amd import signature_verifier_eval as SV
    rig = VT.Rig(V_E, V_PAIRS)
    bt = VT.batch32(V_PAIRS)
    y = bt["labels"].numpy()
    assert set(y.tolist()) == {0.0, 1.0}
    span = dict(zip(rig.names, rig.t.spans))
    (wo, wn), (bo, bn_) = span["classifier.3.weight"], span["classifier.3.bias"]
    sd = VC.torch_state(V_E)
    sd["classifier.3.weight"] = torch.zeros_like(sd["classifier.3.weight"])
    model = SV.SiameseNetwork(V_E)
    row = MARGINS.setdefault(f"verifier/{'contrastive' if use_c else 'bce_only'}", {})
    x1, x2 = bt["x1"].to(VT.DEV), bt["x2"].to(VT.DEV)
    for x0 in V_X0:
        what = f"verifier x0={x0} contrastive={use_c}"
        rig.arenas[0][wo:wo + wn].zero_(); rig.arenas[0][bo:bo + bn_].fill_(x0)
        rig.arenas[1].fill_(7.0)
        met = dict(zip(TC.METRICS, VT.run_grads(rig, bt, use_c).cpu().numpy()))
        p = rig.outputs()["similarity"].numpy()
        logits = np.full(V_PAIRS, x0, np.float32)
        check_p(logits, p, row, what)
        check_mean(met["bce"], H.loss_ref(p, y), row, "bce", what + " bce")
        assert np.isfinite(list(met.values())).all(), met
        if not use_c:
            assert met["contrastive"] == 0.0 and met["loss"] == met["bce"], met
        assert met["n_correct"] == float(((p > 0.5) == (y == 1.0)).sum()), (met, p)
        if x0 == 0.0:
            assert (p == 0.5).all() and met["n_correct"] == float((y == 0.0).sum())       # p == 0.5 predicts 0
        g = rig.views("grads")
        assert all(bool(torch.isfinite(t).all()) for t in g.values()), what
        ref = H.dlogit_ref(p, y, V_PAIRS)
        got_b = float(g["classifier.3.bias"][0])
        bound = ULP * H.spacing32(ref).sum() + (V_PAIRS + 2) * 2.0 ** -24 * np.abs(ref).sum()
        if (ref == 0.0).all():
            assert got_b == 0.0, f"{what}: bias gradient {got_b!r} of a dead head"
        else:
            assert abs(got_b - ref.sum()) <= bound, f"{what}: bias gradient {got_b!r} vs {ref.sum()!r} (bound {bound:.3e})"
            _note(row, "cls3_bias_grad", abs(got_b - ref.sum()) / bound)
        for k in ("classifier.0.weight", "classifier.0.bias") + TC.CONV_BIAS:
            assert bool((g[k] == 0.0).all()), f"{what}: {k} gradient behind a zero classifier.3.weight"
        dead = H.regime(x0, 0).dead
        if dead:
            assert bool((g["classifier.3.weight"] == 0.0).all()), f"{what}: classifier.3.weight gradient of a dead head"
        if not use_c:
            for k, t in g.items():                              # nothing but the head's own bias / weight can carry a gradient
                if dead or not k.startswith("classifier.3."):
                    assert bool((t == 0.0).all()), f"{what}: gradient {k} is not exactly zero"
        else:
            r64, r32 = _verifier_encoder_reference(rig.decisions())
            for k in rig.names:
                if not k.startswith("encoder.") or k in TC.CONV_BIAS:
                    continue
                w64 = r64[k].numpy().reshape(-1)
                scale = float(np.abs(w64).max())
                bnd = min(TC.MARGIN * float(np.abs(r32[k].double().numpy().reshape(-1) - w64).max()) / scale, TC.CAP)
                d = float(np.abs(g[k].double().numpy().reshape(-1) - w64).max()) / scale
                assert d <= bnd, f"{what} grad {k}: relative deviation {d:.3e} exceeds bound {bnd:.3e}"
                _note(row, "encoder_grads", d / bnd)
        # the inference path's score on the same state
        sd["classifier.3.bias"] = torch.full_like(sd["classifier.3.bias"], x0)
        model.load_state_dict(sd, strict=True)
        s = model.to(VT.DEV).eval()(x1, x2)[2].reshape(-1).cpu().numpy()
        assert np.array_equal(s, p), f"{what}: the inference path's score {s} is not the trainer's similarity {p}"
    rig.t.close()
