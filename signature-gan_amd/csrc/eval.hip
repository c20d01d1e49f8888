// eval.hip -- the C ABI's entry points outside a training step: generation, scoring, and the eval-mode gradients of the per-image
// objective with respect to the latents and to the Generator's parameters.  Host code only.
#include "ctx.h"

// What every forward / latent-gradient entry point enqueues on the caller's stream before its own kernels, behind its argument
// checks (a refusal enqueues and invalidates nothing): wait for an abandoned early D(real) forward, then rebuild what the
// arenas' changes made stale.  with_d: the call runs the Discriminator in workspace rows [0, batch) -- what a step carries in
// those rows is dropped, and a spectral-norm context forms sigma into slot 2 first (sn_power_iteration: train(), u and v move
// as under torch's hook; else from the stored u, v) and packs W / sigma.  Generator only: a spectral-norm context's
// Discriminator packs follow sigma, not the arena, and are left alone (d_dirty stays).
static int begin_eval(siggan_ctx* c, hipStream_t s, bool with_d, bool sn_power_iteration) {
    if (with_d) invalidate(c, INV_ROWS);
    const int rc = settle(c, s);
    if (rc) return rc;
    Lanes L(c, s);
    if (with_d) {
        if (c->sn) launch_sn_sigma(c->snt, sn_power_iteration, 2, SN_EPS, s);
        repack(c, L, s, s, c->g_dirty, c->sn || c->d_dirty, 2);
        c->g_dirty = c->d_dirty = false;
    } else {
        repack(c, L, s, s, c->g_dirty, !c->sn && c->d_dirty);
        c->g_dirty = false; if (!c->sn) c->d_dirty = false;
    }
    return SIGGAN_OK;
}

extern "C" int siggan_g_forward(siggan_ctx* c, const float* z_dev, int32_t batch, int32_t training, float* images_dev,
                                void* stream) {
    ENTER(c);
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (training && (rc = check_bn_batch(c, batch))) return rc;
    if (!z_dev || !images_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = begin_eval(c, s, false, false))) return rc;
    GFwdOpt o; o.training = training != 0;
    c->cs.ga_last_B = g_forward_pass(c, z_dev, batch, images_dev, s, o);
    if (training) c->g_dirty = true;   // running statistics moved: the eval-mode tables are stale
    LAUNCHCHK();
    return lane_check(c);
}

extern "C" int siggan_g_generate_u8(siggan_ctx* c, const float* z_dev, int32_t batch, uint8_t* u8_dev, float* images_dev,
                                    int32_t* stats_dev, float threshold, void* stream) {
    ENTER(c);
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (!z_dev || !u8_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (reinterpret_cast<uintptr_t>(u8_dev) & 3) return FAIL(SIGGAN_E_INVALID, "u8_dev must be 4-byte aligned");
    if (stats_dev && !isfinite(threshold)) return FAIL(SIGGAN_E_INVALID, "threshold must be finite");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = begin_eval(c, s, false, false))) return rc;
    GFwdOpt o; o.u8 = u8_dev; o.stats = stats_dev; o.thr = threshold;
    c->cs.ga_last_B = g_forward_pass(c, z_dev, batch, images_dev, s, o);
    LAUNCHCHK();
    return lane_check(c);
}

// The gradient with respect to z of a per-image objective  wr * recon + wd * realism + wp * prior  through the EVAL-mode
// Generator and, for the realism term -max(log D(G(z)), -100), the EVAL-mode Discriminator (no dropout; spectral norm: W / sigma
// from the stored u, v, which do not move).  ONE device sequence serves both entry points: siggan_g_latent_grad is the call with
// the weights (1, 0, 0), its loss in the objective's place, no terms and no probs.  All on the caller's stream:
//   - the Generator forward with every activation kept (g_a): Lg + 2 launches;
//   - [wd > 0]  d_forward_rows at rows [0, B) with stored logits (Ld + 1), the per-image classifier tail k_cls_bwd_eval (1), the
//     Discriminator's input-gradient chain -- launch_gconv form 1 on the d_up packs, EPI_LRELU_BWD without a dropout table
//     (Ld - 1) -- and the first block's input-gradient times 1 - x^2 into dpre (1);
//   - [wr > 0]  k_recon_loss (1): the loss partials and its seed of dpre -- with wd > 0 added onto the Discriminator's as
//     fmaf(wr, ., dpre): no axpy launch;
//   - k_obj_fin_tiles (1): the objective (and terms) per image, and the per-image scale tables below;
//   - the backward through the Generator with BatchNorm as the per-channel affine it is in eval mode -- g . act'(a) . scale[c],
//     none of the training backward's batch sums -- (Lg + 3): the final conv's input-gradient (1), one implicit GEMM per block,
//     fc (2, the prior's wp * z / latent riding in k_fc_dz_sum).  The blocks' input-gradients are launch_gconv form 0 on the packs
//     g_dn[l], as in g_backward_pass, with the EXISTING epilogue EPI_LRELU_BWD: acc * (aref > 0 ? 1 : slope) * noise[n][c] on the
//     stored activation is exactly block l-1's mask and eval scale once `noise` is that block's scale row repeated per image
//     (lg_tab, rebuilt every call: the running statistics move).  Block 0's scale is per feature (F values), so the GEMM into it
//     stores raw values and k_fc_dz applies mask and scale on load.
// 2 Lg + 6 + [wr > 0] + [wd > 0] (2 Ld + 2) launches plus split-K tails.  (1, 0, 0): 2 Lg + 7, which is also siggan_g_latent_grad
// -- 15 at 64x64; (0, 1, 0): 24; all three: 25; the prior alone: Lg + 4, no backward chain (dz = wp * z / latent).
// Scratch: dpre, g_da, partial, partial_b, lg_tab, the activations g_a (the eval forward's to overwrite: Carried::ga_last_B
// says so) and, with wd > 0, the Discriminator's rows [0, B) of d_a and d_dv, logits and dlogit (the realism terms when
// terms_dev is not given) -- all rewritten by a training phase before it reads them, none carried between calls; what a step
// carries in those rows is dropped exactly as siggan_d_forward drops it (begin_eval).
// seed_dev (siggan_g_latent_objective_grad_seeded): a caller-supplied image-space gradient joins dpre behind the two seeds above
// as k_seed_dpre (1) -- fmaf(seed, 1 - x^2, dpre), or seed * (1 - x^2) when nothing is there yet -- and the backward chain runs
// whatever the weights; the objective and the terms never include it.  Null: exactly the sequence above.
// The caller has validated everything: exactly one target when wr > 0 (none otherwise), probs_dev only with wd > 0.
static int latent_objective_grad(siggan_ctx* c, const float* z_dev, int B, const uint8_t* target_u8_dev, const float* target_f32_dev,
                                 float wr, float wd, float wp, float* dz_dev, float* objective_dev, float* terms_dev,
                                 float* probs_dev, float* images_dev, hipStream_t s, const float* seed_dev = nullptr) {
    const int rc = begin_eval(c, s, wd > 0.f, false);
    if (rc) return rc;
    const int Lg = c->Lg, S = c->S;
    const float gs = c->cfg.g_leaky_slope;
    float* const img = images_dev ? images_dev : c->img;
    c->cs.ga_last_B = g_forward_pass(c, z_dev, B, img, s);
    float* const realism = terms_dev ? terms_dev + B : c->dlogit;
    objective_seeds(c, img, B, target_u8_dev, target_f32_dev, wr, wd, realism, probs_dev, s);
    if (seed_dev) launch_seed_dpre(img, seed_dev, c->dpre, B, S, wr > 0.f || wd > 0.f, s);
    ScaleTiles t; memset(&t, 0, sizeof t);
    const float* tab[MAXL + 1] = {nullptr};
    float* next = c->lg_tab;
    for (int l = 1; l < Lg; ++l) {
        t.src[t.nt] = c->g_bne[l]; t.dst[t.nt] = next; t.C[t.nt] = c->gC[l]; ++t.nt;
        tab[l] = next; next += (int64_t)B * c->gC[l];
    }
    launch_obj_fin_tiles(ObjFin{c->partial_b, recon_loss_parts(S), 1.0f / (float)(S * S), realism, z_dev, c->latent, wr, wd, wp,
                                objective_dev, terms_dev}, B, t, s);
    if (wr > 0.f || wd > 0.f || seed_dev) {
        launch_final_dgrad_eval(c->dpre, c->wfin_t, (const float*)c->g_a[Lg], c->g_bne[Lg], (float*)c->g_da[Lg], B, S, gs, s);
        for (int l = Lg; l >= 1; --l) {
            GConvArgs a = gconv_args(c, 0, B, 4 << l, c->gC[l], c->gC[l - 1]);
            a.in = c->g_da[l]; a.wp = c->g_dn[l]; a.out = c->g_da[l - 1]; a.epi = EPI_RAW;
            if (l >= 2) { a.epi = EPI_LRELU_BWD; a.aref = c->g_a[l - 1]; a.noise = tab[l - 1]; a.slope = gs; }
            launch_gconv(a, s);
        }
        // (the last 64 floats of `partial` are siggan_op_adam's scratch slot; the cap is restated in tests/evalpaths.py)
        launch_fc_dz((const float*)c->g_da[0], (const float*)c->g_a[0], c->g_bne[0], GP(c, gi_fc_w()), dz_dev, c->partial,
                     PARTIAL_FLOATS - 64, B, c->latent, c->gC[0], gs, s, wp > 0.f ? z_dev : nullptr, wp / (float)c->latent);
    } else {
        launch_prior_dz(z_dev, dz_dev, (int64_t)B * c->latent, wp / (float)c->latent, s);   // the prior alone: dz = wp * z / latent
    }
    LAUNCHCHK();
    return lane_check(c);
}
// The tensor checks every objective entry point ends its refusals with (same order, same texts, nothing enqueued).
static int check_latent_tensors(const siggan_ctx* c, const float* z_dev, const float* dz_dev, const float* out_dev,
                                const uint8_t* target_u8_dev, const float* target_f32_dev, const float* images_dev) {
    if (!z_dev || !dz_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (reinterpret_cast<uintptr_t>(target_u8_dev) & 3) return FAIL(SIGGAN_E_INVALID, "target_u8_dev must be 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(target_f32_dev) | reinterpret_cast<uintptr_t>(images_dev)) & 15)
        return FAIL(SIGGAN_E_INVALID, "target_f32_dev and images_dev must be 16-byte aligned");
    if (c->cs.g_fwd_pending)
        return FAIL(SIGGAN_E_STATE, "siggan_step_begin must be followed by siggan_g_grads first: the pipelined forward's activations are in use");
    return SIGGAN_OK;
}

// The checks the four objective entry points share ahead of check_latent_tensors, in their one order; `own`: what the entry point
// itself refuses between the weights' values and the target count.  The next term of the objective is checked here, once.
template <class Own>
static int check_objective(siggan_ctx* c, const char* entry, int batch, const siggan_latent_objective* w, const uint8_t* target_u8_dev,
                           const float* target_f32_dev, const float* probs_dev, Own own) {
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (c->dt != DT_F32) return FAIL(SIGGAN_E_INVALID, "%s needs an fp32 context (16-bit activations are not built for it)", entry);
    if (!w) return FAIL(SIGGAN_E_INVALID, "null weights");
    const float wr = w->recon_weight, wd = w->realism_weight, wp = w->prior_weight;
    if (!isfinite(wr) || !isfinite(wd) || !isfinite(wp) || wr < 0.f || wd < 0.f || wp < 0.f)
        return FAIL(SIGGAN_E_INVALID, "the objective's weights must be finite and >= 0, got (%g, %g, %g)", (double)wr, (double)wd, (double)wp);
    if ((rc = own())) return rc;
    const int ntargets = (target_u8_dev != nullptr) + (target_f32_dev != nullptr);
    if (wr > 0.f && ntargets != 1)
        return FAIL(SIGGAN_E_INVALID, "recon_weight > 0 needs exactly one of target_u8_dev and target_f32_dev");
    if (wr == 0.f && ntargets != 0) return FAIL(SIGGAN_E_INVALID, "a target was given but recon_weight is 0");
    if (probs_dev && wd == 0.f) return FAIL(SIGGAN_E_INVALID, "probs_dev needs realism_weight > 0");
    return SIGGAN_OK;
}

extern "C" int siggan_g_latent_grad(siggan_ctx* c, const float* z_dev, int32_t batch, const uint8_t* target_u8_dev,
                                    const float* target_f32_dev, float* dz_dev, float* loss_dev, float* images_dev, void* stream) {
    ENTER(c);
    const siggan_latent_objective w = {1.f, 0.f, 0.f};             // the reconstruction term alone; its own text for the target count
    int rc = check_objective(c, __func__, batch, &w, target_u8_dev, target_f32_dev, nullptr, [&] {
        return (target_u8_dev != nullptr) == (target_f32_dev != nullptr) ? FAIL(SIGGAN_E_INVALID, "exactly one of target_u8_dev and target_f32_dev must be given") : 0; });
    if (rc || (rc = check_latent_tensors(c, z_dev, dz_dev, loss_dev, target_u8_dev, target_f32_dev, images_dev))) return rc;
    return latent_objective_grad(c, z_dev, batch, target_u8_dev, target_f32_dev, 1.f, 0.f, 0.f, dz_dev, loss_dev, nullptr, nullptr,
                                 images_dev, (hipStream_t)stream);
}

extern "C" int siggan_g_latent_objective_grad(siggan_ctx* c, const float* z_dev, int32_t batch, const uint8_t* target_u8_dev,
                                              const float* target_f32_dev, const siggan_latent_objective* w, float* dz_dev,
                                              float* objective_dev, float* terms_dev, float* probs_dev, float* images_dev,
                                              void* stream) {
    ENTER(c);
    int rc = check_objective(c, __func__, batch, w, target_u8_dev, target_f32_dev, probs_dev, [&] {
        return w->recon_weight == 0.f && w->realism_weight == 0.f && w->prior_weight == 0.f ? FAIL(SIGGAN_E_INVALID, "all three weights of the objective are 0") : 0; });
    if (rc || (rc = check_latent_tensors(c, z_dev, dz_dev, objective_dev, target_u8_dev, target_f32_dev, images_dev))) return rc;
    return latent_objective_grad(c, z_dev, batch, target_u8_dev, target_f32_dev, w->recon_weight, w->realism_weight, w->prior_weight,
                                 dz_dev, objective_dev, terms_dev, probs_dev, images_dev, (hipStream_t)stream);
}

extern "C" int siggan_g_latent_objective_grad_seeded(siggan_ctx* c, const float* z_dev, int32_t batch, const uint8_t* target_u8_dev,
                                                     const float* target_f32_dev, const siggan_latent_objective* w,
                                                     const float* image_grad_dev, float* dz_dev, float* objective_dev,
                                                     float* terms_dev, float* probs_dev, float* images_dev, void* stream) {
    ENTER(c);
    int rc = check_objective(c, __func__, batch, w, target_u8_dev, target_f32_dev, probs_dev, [&] {
        if (!image_grad_dev) return FAIL(SIGGAN_E_INVALID, "null image_grad_dev (use siggan_g_latent_objective_grad without a seed)");
        return reinterpret_cast<uintptr_t>(image_grad_dev) & 15 ? FAIL(SIGGAN_E_INVALID, "image_grad_dev must be 16-byte aligned") : 0; });
    if (rc || (rc = check_latent_tensors(c, z_dev, dz_dev, objective_dev, target_u8_dev, target_f32_dev, images_dev))) return rc;
    return latent_objective_grad(c, z_dev, batch, target_u8_dev, target_f32_dev, w->recon_weight, w->realism_weight, w->prior_weight,
                                 dz_dev, objective_dev, terms_dev, probs_dev, images_dev, (hipStream_t)stream, image_grad_dev);
}

// The gradient with respect to the Generator's PARAMETERS of the same per-image objective (prior weight 0: it does not depend
// on them), summed over the batch, into a caller-owned arena-shaped buffer.  Both networks in eval mode; BatchNorm is the fixed
// per-channel affine of its running statistics, so one sample is fine and nothing moves.  All on the caller's stream:
//   - the Generator forward in the training forward's SHAPE with the eval tables (g_forward_pass keep_y): fc folded (1), per
//     block the raw GEMM into g_y[l] and k_bn_relu with g_bne[l] (2 Lg), the final conv (1) -- the folded forward's expression
//     on the same accumulators, every activation g_a and every pre-BatchNorm tensor g_y[1..Lg] kept: 2 Lg + 2 launches;
//   - objective_seeds: [wd > 0] 2 Ld + 2, [wr > 0] 1;  k_obj_fin_tiles without tiles (1);
//   - the final conv's weight / bias gradient from dpre and g_a[Lg] (2);
//   - [first_layer <= Lg]  the final conv's input-gradient through the last activation with a scale row of ones (1): dpost[Lg];
//     then for l = Lg .. max(first_layer, 1): k_bn_eval_bwd + k_part_sum (2: dgamma, dbeta, g_da[l] becomes dy = scale * dpost),
//     k_wgrad on (g_a[l-1], g_da[l]) as in g_backward_pass (1), and, while l > first_layer, the input-gradient GEMM on g_dn[l]
//     into g_da[l-1] (1) -- EPI_LRELU_BWD on the stored activation without a table (the mask alone: dpost[l-1]) for l >= 2, raw
//     into block 0;
//   - [first_layer == 0]  k_fc_bn_eval_bwd (1: the BatchNorm1d sums, g_da[0] becomes d(fc output)) and k_fc_wgrad (1);
//   - [first_layer > 0]  one memset node over the frozen prefix of dparams.
// With nb = Lg - max(first_layer, 1) + 1 trainable blocks (0 for first_layer = Lg + 1) and nd = Lg - first_layer input-gradient
// GEMMs (Lg for first_layer 0, 0 for Lg + 1):  2 Lg + 5 + [wr > 0] + [wd > 0] (2 Ld + 2) + [first_layer <= Lg] (1 + 3 nb + nd)
// + [first_layer == 0] 2 launches plus split-K tails; at 64x64 with the weights (1, 0): 33 for first_layer 0, 22 for 3, 14 for 5.
// Of these the implicit GEMMs and weight gradients (what siggan_prof_* counts): Lg + [wd > 0] 2 (Ld - 1) + nb + nd.
// Scratch: what latent_objective_grad uses (dpre, g_da, partial, partial_b, the activations g_a, with wd > 0 the Discriminator's
// rows [0, B), logits, dlogit) plus g_y[1..Lg], slab (the weight-gradient slabs, the final conv's partial rows) and probs (the
// objective when objective_dev is not given) -- all rewritten by a training phase before it reads them, none carried between
// calls.  Carried: ga_last_B = 0 (every activation was materialised), lP[0] as d_forward_rows left it, and begin_eval's
// invalidate(INV_ROWS) with wd > 0, exactly as latent_objective_grad.
static int param_grad(siggan_ctx* c, const float* z_dev, int B, const uint8_t* target_u8_dev, const float* target_f32_dev, float wr,
                      float wd, int fl, float* dparams, float* objective_dev, float* terms_dev, float* probs_dev, float* images_dev,
                      hipStream_t s) {
    const int rc = begin_eval(c, s, wd > 0.f, false);
    if (rc) return rc;
    const int Lg = c->Lg, S = c->S;
    const float gs = c->cfg.g_leaky_slope;
    float* const img = images_dev ? images_dev : c->img;
    GFwdOpt o; o.keep_y = true;
    c->cs.ga_last_B = g_forward_pass(c, z_dev, B, img, s, o);
    float* const realism = terms_dev ? terms_dev + B : c->dlogit;
    objective_seeds(c, img, B, target_u8_dev, target_f32_dev, wr, wd, realism, probs_dev, s);
    ScaleTiles t; memset(&t, 0, sizeof t);
    launch_obj_fin_tiles(ObjFin{c->partial_b, recon_loss_parts(S), 1.0f / (float)(S * S), realism, z_dev, c->latent, wr, wd, 0.f,
                                objective_dev ? objective_dev : c->probs, terms_dev}, B, t, s);
    auto G_ = [&](int i) { return dparams + c->g_off[i]; };
    bool ok = launch_final_wgrad_eval(c->dpre, (const float*)c->g_a[Lg], c->slab, c->slab_floats, G_(gi_fin_w(c)), G_(gi_fin_b(c)), B, S, s);
    if (fl <= Lg) {
        launch_final_dgrad_eval(c->dpre, c->wfin_t, (const float*)c->g_a[Lg], c->ones, (float*)c->g_da[Lg], B, S, gs, s);
        for (int l = Lg; l >= (fl > 1 ? fl : 1); --l) {
            const int Hi = 4 << (l - 1), Ho = 2 * Hi, Ci = c->gC[l - 1], Co = c->gC[l];
            // (the last 64 floats of `partial` are siggan_op_adam's scratch slot)
            ok = launch_bn_eval_bwd((float*)c->g_da[l], (const float*)c->g_y[l], (int64_t)B * Ho * Ho, Co, c->g_bne[l], c->partial,
                                    PARTIAL_FLOATS - 64, G_(gi_bn_w(l)), G_(gi_bn_b(l)), s) && ok;
            const WgradCall g = wgrad_args(c, c->g_a[l - 1], c->g_da[l], G_(gi_up_w(l)), c->slab, B, Hi, Ci, Co);
            launch_wgrad(g.w, g.max_splits, s);
            if (l > fl) {
                GConvArgs a = gconv_args(c, 0, B, Ho, Co, Ci);
                a.in = c->g_da[l]; a.wp = c->g_dn[l]; a.out = c->g_da[l - 1]; a.epi = EPI_RAW;
                if (l >= 2) { a.epi = EPI_LRELU_BWD; a.aref = c->g_a[l - 1]; a.noise = nullptr; a.slope = gs; }
                launch_gconv(a, s);
            }
        }
    }
    if (fl == 0) {
        launch_fc_bn_eval_bwd((float*)c->g_da[0], (const float*)c->g_a[0], c->g_bne[0], GP(c, gi_fc_w()), GP(c, gi_fc_b()), z_dev,
                              G_(gi_bn0_w()), G_(gi_bn0_b()), B, c->latent, c->gC[0], gs, s);
        launch_fc_wgrad(c->dt, c->g_da[0], z_dev, G_(gi_fc_w()), G_(gi_fc_b()), B, c->latent, c->gC[0], s);
    } else {      // the frozen layers' spans: a prefix of the arena
        const int first = fl > Lg ? gi_fin_w(c) : gi_up_w(fl);
        HIPCHK(hipMemsetAsync(dparams, 0, (size_t)c->g_off[first] * sizeof(float), s));
    }
    if (!ok) return FAIL(SIGGAN_E_STATE, "siggan_g_param_grad: a reduction's partial rows had no carve (batch too large for the workspace)");
    LAUNCHCHK();
    return lane_check(c);
}

extern "C" int siggan_g_param_grad(siggan_ctx* c, const float* z_dev, int32_t batch, const uint8_t* target_u8_dev,
                                   const float* target_f32_dev, const siggan_latent_objective* w, int32_t first_layer,
                                   float* dparams_dev, float* objective_dev, float* terms_dev, float* probs_dev, float* images_dev,
                                   void* stream) {
    ENTER(c);
    int rc = check_objective(c, __func__, batch, w, target_u8_dev, target_f32_dev, probs_dev, [&] {
        if (w->prior_weight != 0.f)
            return FAIL(SIGGAN_E_INVALID, "prior_weight must be 0: the prior does not depend on the parameters, got %g", (double)w->prior_weight);
        return w->recon_weight == 0.f && w->realism_weight == 0.f ? FAIL(SIGGAN_E_INVALID, "both weights of the objective are 0") : 0; });
    if (rc) return rc;
    if (first_layer < 0 || first_layer > c->Lg + 1)
        return FAIL(SIGGAN_E_INVALID, "first_layer %d outside [0, %d]", first_layer, c->Lg + 1);
    if (reinterpret_cast<uintptr_t>(dparams_dev) & 15) return FAIL(SIGGAN_E_INVALID, "dparams_dev must be 16-byte aligned");
    if ((rc = check_latent_tensors(c, z_dev, dparams_dev, dparams_dev, target_u8_dev, target_f32_dev, images_dev))) return rc;
    return param_grad(c, z_dev, batch, target_u8_dev, target_f32_dev, w->recon_weight, w->realism_weight, first_layer, dparams_dev,
                      objective_dev, terms_dev, probs_dev, images_dev, (hipStream_t)stream);
}

extern "C" int siggan_d_forward(siggan_ctx* c, const float* x_dev, int32_t batch, int32_t training, const float* masks_dev,
                                float* probs_dev, float* features_dev, void* stream) {
    ENTER(c);
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (!x_dev || (!probs_dev && !features_dev)) return FAIL(SIGGAN_E_INVALID, "null tensor");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = begin_eval(c, s, true, training != 0))) return rc;       // rows [0, batch) are overwritten
    const bool drop = training != 0 && c->cfg.dropout > 0.f;
    if (drop) { if (!masks_dev) launch_tick(c->dev, s); make_noise(c, masks_dev, batch, 0, 1, s); }
    DFwdOpt o; o.dropout = drop;
    c->cs.lP[0] = d_forward_rows(c, x_dev, 0, batch, s, c->slab_k, o);
    if (probs_dev) launch_bce(LogitSrc{c->logits}, batch, batch, 0.f, 0.f, probs_dev, nullptr, nullptr, 0, s);
    if (features_dev) launch_cls_features(c->dt, c->d_a[c->Ld], features_dev, batch, c->dC[c->Ld], s);
    LAUNCHCHK();
    return lane_check(c);
}

extern "C" int siggan_d_score_u8(siggan_ctx* c, const uint8_t* u8_dev, int32_t batch, int32_t binarize, float* probs_dev,
                                 float* x_dev, void* stream) {
    ENTER(c);
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (!u8_dev || !probs_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (binarize < -1 || binarize > 255) return FAIL(SIGGAN_E_INVALID, "binarize must be -1 (off) or a byte value, got %d", binarize);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = begin_eval(c, s, true, false))) return rc;               // as siggan_d_forward(training = 0)
    DFwdOpt o; o.u8 = u8_dev; o.binarize = binarize; o.x_out = x_dev;
    c->cs.lP[0] = d_forward_rows(c, nullptr, 0, batch, s, c->slab_k, o);
    launch_bce(LogitSrc{c->logits}, batch, batch, 0.f, 0.f, probs_dev, nullptr, nullptr, 0, s);
    LAUNCHCHK();
    return lane_check(c);
}
