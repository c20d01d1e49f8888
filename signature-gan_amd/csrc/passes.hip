// passes.hip -- the engine's internal passes: the job tables of what is derived from the arenas, the implicit GEMMs' geometry, and
// both networks' forward / backward passes, which step.hip and eval.hip put together.  Host code only: no kernel, no launch.
#include "ctx.h"

// 1 / sigma of spectral-norm layer `layer` as pass `slot` left it (null without spectral norm): what a D pack is scaled by
static const float* sn_inv_sigma(const siggan_ctx* c, int slot, int layer) {
    return c->sn ? c->sn_sig + (slot * 2 + 1) * SnTable::MAXS + layer : nullptr;
}
// k_prepare's jobs of network `which` from its records (struct Derived).  Job order: by kind, arena order within a kind.
static void prep_table(const siggan_ctx* c, int which, int sn_slot, PrepTable& t) {
    t.njobs = 0; t.overflow = 0;
    const float* P = which == 0 ? c->st.g_params : c->st.d_params;
    for (int kind : {DV_FC, DV_CONV, DV_T16, DV_BN, DV_TAPS})
        for (const Derived& r : c->rec[which]) {
            if (r.kind != kind || !r.dst) continue;
            PrepJob j; memset(&j, 0, sizeof j);
            j.src = P + r.off; j.dst = r.dst;
            if (which == 1) j.mul = sn_inv_sigma(c, sn_slot, r.layer - 1);   // W / sigma of this pass
            if (kind == DV_CONV) {
                j.dt = c->dt;
                PrepJob up = j;
                j.type = PREP_PACK_DOWN; j.O = r.A; j.I = r.Bc;
                up.type = PREP_PACK_UP; up.I = r.A; up.O = r.Bc; up.dst = r.dst2;
                prep_add(t, which == 0 ? up : j);                            // the forward pass's pack first
                prep_add(t, which == 0 ? j : up);
                continue;
            }
            if (kind == DV_FC) { j.type = PREP_FC_T; j.O = r.A; j.I = r.Bc; }
            else if (kind == DV_T16) { j.type = PREP_CLS; j.O = r.A; }
            else if (kind == DV_BN) {
                j.type = PREP_BN_EVAL; j.O = r.A; j.perm = r.Bc; j.src2 = P + r.off2;
                j.src3 = c->st.g_bn_running_mean + r.bn_off; j.src4 = c->st.g_bn_running_var + r.bn_off;
            } else {
                if (r.dst2) { PrepJob sc = j; sc.type = PREP_SCALE; sc.O = (int)r.n; sc.dst = r.dst2; prep_add(t, sc); }
                j.type = PREP_TAPS; j.O = r.A; j.I = r.Bc;
            }
            prep_add(t, j);
        }
}
// One launch per network rebuilds everything derived from its arena.  sg / sd: the lanes the two launches go to.
// conv1_x != nullptr (G step, no spectral norm): the D table's launch also runs the first-block forward of conv1_B images at
// conv1_x into workspace rows [conv1_r0, ...) -- it reads the raw block-1 weights, not a pack (launch_prepare_conv1)
void siggan::repack(const siggan_ctx* c, Lanes& L, hipStream_t sg, hipStream_t sd, bool do_g, bool do_d, int sn_slot, const float* conv1_x,
                    int conv1_r0, int conv1_B) {
    PrepTable t;
    if (do_g) {
        prep_table(c, 0, 0, t);
        if (!launch_prepare(t, BN_EPS, sg)) L.note(hipErrorInvalidValue);          // table overflow: reported by the caller
    }
    if (do_d) {
        prep_table(c, 1, sn_slot, t);
        bool ok;
        if (conv1_x && !c->sn) {
            const int64_t H = c->S >> 1;
            char* out = c->d_a[1] + (size_t)((int64_t)conv1_r0 * H * H * c->dC[1]) * c->es;
            ok = launch_prepare_conv1(t, BN_EPS, c->dt, conv1_x, DP(c, di_w(1)), DP(c, di_b(1)), c->cfg.leaky_slope, out, conv1_B, c->S, sd);
        } else {
            ok = launch_prepare(t, BN_EPS, sd);
        }
        if (!ok) L.note(hipErrorInvalidValue);
    }
}
// k_adam_pack's jobs of network `which` (c->packable[which]) from the same records: the whole arena, record by record, so
// the Discriminator's block 1 -- what the nride riders read -- comes first
void siggan::ap_table(const siggan_ctx* c, int which, int nride, ApTable& t) {
    t.njobs = 0; t.overflow = 0;
    for (const Derived& r : c->rec[which]) {
        ApJob j; memset(&j, 0, sizeof j);
        j.off = r.off; j.dst = r.dst;
        if (r.kind == DV_FLAT || r.kind == DV_FC) { j.type = AP_FLAT; j.n = r.n + r.n2; ap_add(t, j); continue; }
        j.A = r.A; j.Bc = r.Bc;
        if (r.kind == DV_CONV) { j.type = AP_CONV; j.dt = c->dt; j.dst2 = r.dst2; }
        else if (r.kind == DV_T16) j.type = AP_T16;
        else if (r.kind == DV_BN) {
            j.type = AP_BN; j.off2 = r.off2;
            j.rmean = c->st.g_bn_running_mean + r.bn_off; j.rvar = c->st.g_bn_running_var + r.bn_off;
        } else { j.type = AP_TAPS; j.n = r.n; j.off2 = r.off2; j.n2 = r.n2; j.wait = nride; }
        ap_add(t, j);
    }
}

// The ONE place the geometry of a 4x4 stride-2 implicit GEMM is derived.  form 0 ("down", a stride-2 convolution or the input-
// gradient of a transposed one): h_in -> h_in / 2; form 1 ("up", a transposed convolution or the input-gradient of a stride-2
// one): h_in -> 2 h_in.  A GEMM row is a pixel of the SMALL side in both forms.  The caller sets in / wp / out, the epilogue
// fields, and slab where it runs beside another GEMM.
GConvArgs siggan::gconv_args(const siggan_ctx* c, int form, int B, int h_in, int c_in, int c_out) {
    GConvArgs a; memset(&a, 0, sizeof a);
    a.dt = c->dt; a.gslope = c->cfg.g_leaky_slope;
    a.slab = c->slab_k; a.slab_floats = c->slab_k_floats; a.zeros = c->zeros;
    const int h_small = form == 0 ? h_in / 2 : h_in;
    a.form = form; a.B = B; a.Hi = a.Wi = h_in; a.Ci = c_in; a.Co = c_out;
    a.Ho = a.Wo = form == 0 ? h_in / 2 : 2 * h_in;
    a.lgHr = a.lgWr = ilog2(h_small); a.M = B * h_small * h_small;
    return a;
}
// ... and of its weight gradient: small [B][h_small]^2[c_small] x large [B][2 h_small]^2[c_large] -> dw, split over the pixels
// into as many slabs as `slab` (slab_floats, every weight-gradient slab region has that size) holds.  db stays the caller's.
WgradCall siggan::wgrad_args(const siggan_ctx* c, const void* small, const void* large, float* dw, float* slab, int B, int h_small,
                            int c_small, int c_large) {
    WgradCall g; memset(&g, 0, sizeof g);
    WgradArgs& w = g.w;
    w.zeros = c->zeros; w.dt = c->dt;
    w.S = small; w.L = large; w.slab = slab; w.dw = dw; w.B = B; w.Cs = c_small; w.Cl = c_large;
    w.lgHs = w.lgWs = ilog2(h_small); w.lgCl = ilog2(c_large); w.K = B * h_small * h_small;
    g.max_splits = (int)(c->slab_floats / ((int64_t)c_small * (16 * c_large + 1)));
    return g;
}

// Generator.forward (generator_vanilla_gan.py:189-209).  training: BN batch stats (+ running
// update) and raw pre-BN outputs kept for the backward pass; eval: BN folded into the epilogue.
// z == nullptr: the latent batch is drawn inside the fc kernel from RNG stream rng_sid and left in z_out (GFwdOpt, ctx.h).
// Returns what Carried::ga_last_B becomes: B after a training forward (its last activation was not written), else 0.
int siggan::g_forward_pass(const siggan_ctx* c, const float* z, int B, float* img, hipStream_t s, const GFwdOpt& o) {
    float* const partial = o.partial ? o.partial : c->partial;
    char* const* const A = o.training ? c->g_a : c->g_ae;     // (fp32: the same buffers)
    const float gs = c->cfg.g_leaky_slope;                   // the Generator's activation: 0 = ReLU, else LeakyReLU(gs)
    // fc + BatchNorm1d + activation: one MFMA launch (fc.hip) whenever the shape allows, else the generic kernels
    if (c->fc_fused && launch_fc_fwd_fused(c->dt, z, GP(c, gi_fc_w()), GP(c, gi_fc_b()), c->fc_y, A[0], GP(c, gi_bn0_w()),
                                          GP(c, gi_bn0_b()), c->st.g_bn_running_mean, c->st.g_bn_running_var, c->st.g_bn_batches,
                                          c->g_bn[0], o.training ? nullptr : c->g_bne[0], o.z_out, c->dev, o.rng_sid, B, c->latent,
                                          c->gC[0], BN_MOMENTUM, BN_EPS, gs, s)) {
    } else if (!o.training) {     // eval: BatchNorm1d + activation folded into the fc epilogue
        launch_fc_fwd(c->dt, z, c->wfc_t, GP(c, gi_fc_b()), A[0], B, c->latent, c->gC[0], gs, s, c->g_bne[0], c->dev, o.rng_sid, o.z_out);
    } else {
        launch_fc_fwd(c->dt, z, c->wfc_t, GP(c, gi_fc_b()), c->fc_y, B, c->latent, c->gC[0], gs, s, nullptr, c->dev, o.rng_sid, o.z_out);
        launch_bn_train_stats(c->dt, c->fc_y, B, c->F, GP(c, gi_bn0_w()), GP(c, gi_bn0_b()), c->st.g_bn_running_mean,
                              c->st.g_bn_running_var, c->st.g_bn_batches, c->g_bn[0], partial, c->gC[0], BN_MOMENTUM,
                              BN_EPS, s);
        launch_bn_relu(c->dt, c->fc_y, A[0], B, c->F, c->g_bn[0], gs, s);
    }
    for (int l = 1; l <= c->Lg; ++l) {
        const int Hi = 4 << (l - 1), C = c->gC[l];
        GConvArgs a = gconv_args(c, 1, B, Hi, c->gC[l - 1], C);
        if (o.slab_k) a.slab = o.slab_k;
        a.in = A[l - 1]; a.wp = c->g_up[l];
        const int64_t off = c->g_bn_off[l];
        if (o.training) {
            a.out = c->g_y[l]; a.epi = EPI_RAW;
            launch_gconv(a, s);
            const int64_t R = (int64_t)B * 4 * Hi * Hi;
            // the LAST block's activation has two readers, the final conv here and its weight gradient in the backward
            // pass: both re-derive it from y and this table, so it is never written (33.5 MB each way at batch 64)
            launch_bn_train_stats(c->dt, c->g_y[l], R, C, GP(c, gi_bn_w(l)), GP(c, gi_bn_b(l)), c->st.g_bn_running_mean + off,
                                  c->st.g_bn_running_var + off, c->st.g_bn_batches + l, c->g_bn[l], partial, 0,
                                  BN_MOMENTUM, BN_EPS, s);
            if (l < c->Lg) launch_bn_relu(c->dt, c->g_y[l], A[l], R, C, c->g_bn[l], gs, s);
        } else if (o.keep_y) {      // (g_bne[l] begins [scale | shift], the two rows k_bn_relu reads: the folded epilogue's expression)
            a.out = c->g_y[l]; a.epi = EPI_RAW;
            launch_gconv(a, s);
            launch_bn_relu(c->dt, c->g_y[l], A[l], (int64_t)B * 4 * Hi * Hi, C, c->g_bne[l], gs, s);
        } else {
            a.out = A[l]; a.epi = EPI_AFFINE_RELU; a.scale = c->g_bne[l]; a.shift = c->g_bne[l] + C;
            launch_gconv(a, s);
        }
    }
    if (o.training)
        launch_final_fwd(c->dt, c->g_y[c->Lg], c->wfin_t, GP(c, gi_fin_b(c)), img, B, c->S, c->gC[c->Lg], gs, s, c->g_bn[c->Lg], o.done);
    else
        launch_final_fwd(c->dt, A[c->Lg], c->wfin_t, GP(c, gi_fin_b(c)), img, B, c->S, c->gC[c->Lg], gs, s, nullptr, o.done, o.u8, o.stats, o.thr);
    return o.training ? B : 0;
}

// Discriminator conv blocks + classifier logits for nB images written to workspace rows
// [r0, r0 + nB) (the D step runs D(real) into rows [0,B) on a side lane while the Generator
// produces the fakes, then D(fake) into rows [B,2B); backward treats the 2B rows as one batch).
// Returns the form the logits were left in: P > 0 partial dot products per image in lparts, 0: stored in `logits`.
int siggan::d_forward_rows(const siggan_ctx* c, const float* x, int r0, int nB, hipStream_t s, float* slab_k, const DFwdOpt& o) {
    const float slope = c->cfg.leaky_slope;
    int P = 0;
    auto act = [&](int l) { const int64_t H = c->S >> l; return c->d_a[l] + (size_t)((int64_t)r0 * H * H * c->dC[l]) * c->es; };
    auto nz = [&](int l) { return o.dropout ? c->d_noise[l] + (int64_t)r0 * c->dC[l] : nullptr; };
    if (o.u8)                   // siggan_d_score_u8: the same block fed from bytes (eval mode: no dropout multipliers)
        launch_conv1_fwd_u8(c->dt, Conv1U8{o.u8, c->deq_lut, o.x_out, o.binarize}, c->sn ? c->d_w1s : DP(c, di_w(1)), DP(c, di_b(1)), slope,
                            act(1), nB, c->S, c->dC[1], s);
    else if (!o.conv1_done)     // (done: it rode in the launch that re-packed D's weights, see repack)
        launch_conv1_fwd(c->dt, x, nB, x, c->sn ? c->d_w1s : DP(c, di_w(1)), DP(c, di_b(1)), nz(1), slope, act(1), nB, c->S, c->dC[1], s);
    for (int l = 2; l <= c->Ld; ++l) {
        GConvArgs a = gconv_args(c, 0, nB, c->S >> (l - 1), c->dC[l - 1], c->dC[l]);
        a.slab = slab_k;
        a.in = act(l - 1); a.wp = c->d_dn[l]; a.out = act(l);
        a.epi = EPI_BIAS_LRELU_DROP; a.bias = DP(c, di_b(l)); a.noise = nz(l); a.slope = slope;
        // fuse_cls (the step phases, whose k_bce / k_cls_bwd read either form): when the last block ends in a split-K epilogue,
        // the classifier's dot product rides there as P partials per image and k_cls_fwd is not launched
        const int P_max = c->dC[c->Ld] * 16 / 1024;
        if (l == c->Ld && o.fuse_cls && P_max >= 1 && P_max <= 16) { a.cls_w = c->wcp; a.cls_part = c->lparts + (size_t)r0 * P_max; }
        const int splits = launch_gconv(a, s);
        if (l == c->Ld && a.cls_w) P = splits;
    }
    if (P == 0)
        launch_cls_fwd(c->dt, act(c->Ld), c->wcp, DP(c, di_cls_b(c)), c->logits + r0, nB, c->dC[c->Ld] * 16, s);
    return P;
}

// Backward through the Discriminator from d(logit).  want_wgrad: fill the D gradient arena
// (D step); want_dimage: continue to d(pre-tanh image) (G step).  The chain of input-gradients
// runs on lane m; each block's weight gradient (lane a) and bias gradient (lane b) only need that
// block's d(pre-activation) and run beside the rest of the chain.
// r0 / garena (spectral norm: one pass at a time): the Bd rows start at workspace row r0 and the gradients go to garena
// (an arena-shaped temporary) instead of the bound arena.  P: the form d_forward_rows left these rows' logits in (< 0: the
// two halves of a 2B-row pass disagree).  Returns whether the tail's all-reduce was started (Carried::early_ar).
bool siggan::d_backward_pass(const siggan_ctx* c, Lanes& L, const float* x0, int n0, const float* x1, int Bd, bool dropout,
                            bool want_wgrad, bool want_dimage, const BceSpec& bce, int P, int r0, float* garena,
                             bool early_allreduce) {
    bool early_ar = false;
    const float slope = c->cfg.leaky_slope;
    const int Ld = c->Ld;
    float* const ga = garena ? garena : c->st.d_grads;
    auto G_ = [&](int i) { return ga + c->d_off[i]; };
    auto act = [&](int l) { const int64_t H = c->S >> l; return c->d_a[l] + (size_t)((int64_t)r0 * H * H * c->dC[l]) * c->es; };
    auto dvp = [&](int l) { const int64_t H = c->S >> l; return c->d_dv[l] + (size_t)((int64_t)r0 * H * H * c->dC[l]) * c->es; };
    auto nz = [&](int l) { return dropout ? c->d_noise[l] + (int64_t)r0 * c->dC[l] : nullptr; };
    // sigmoid + BCE: losses / means into the metrics, d(logit) for the classifier's weight gradient -- on lane b; the
    // chain below recomputes d(logit) from the logits and does not wait for it
    // Lanes: an event record on the main lane delays the kernel behind it by ~6 us and a join whose event
    // completes just before it is waited for costs ~15 us, so a side lane must carry enough work to pay for its fork and
    // join.  D step: the weight gradients (lane a: they overlap the input-gradient chain, putting them on the main lane costs
    // 3 %) and the small reductions (lane b).  G step: nothing here is worth a lane -- the 5 us loss kernel stays on m.
    hipStream_t const sb = want_wgrad ? L.b : L.m;
    // the logits of the rows this pass covers: stored, or P partial dot products per image (d_forward_rows).  Both halves of a
    // 2B-row pass were produced with the same batch size, hence in the same form
    if (P < 0) { L.note(hipErrorInvalidValue); return false; }       // (cannot happen: reported, not computed wrongly)
    const LogitSrc src{c->logits + r0, P ? c->lparts + (size_t)r0 * P : nullptr, P, DP(c, di_cls_b(c))};
    if (sb != L.m) {
        L.fork(L.b);
        launch_bce(src, Bd, bce.n0, bce.y0, bce.y1, c->probs + r0, c->dlogit + r0, bce.mt, bce.is_g, sb, c->gscale);
    }
    // (G step: the loss kernel's work is one more block of the classifier's input-gradient kernel -- one launch, not two)
    const BceRider rider{c->probs + r0, c->dlogit + r0, bce.mt, bce.is_g};
    launch_cls_bwd(c->dt, src, bce.n0, bce.y0, bce.y1, c->wcp, act(Ld), nz(Ld), slope, dvp(Ld), Bd, c->dC[Ld], L.m, c->gscale,
                   sb == L.m ? &rider : nullptr);
    if (want_wgrad)
        launch_cls_wgrad(c->dt, c->dlogit + r0, act(Ld), G_(di_cls_w(c)), G_(di_cls_b(c)), Bd, c->dC[Ld], sb);
    for (int l = Ld; l >= 2; --l) {
        const int Ho = c->S >> l, Co = c->dC[l], Ci = c->dC[l - 1];
        // 16-bit contexts (launch-latency-bound): the LAST block's weight gradient runs behind the input-gradient chain on the
        // main lane, own slab, so that lane a ends before the main lane does (measured with the three 16-bit lane rules
        // together: bf16 0.718 -> 0.707 ms; at fp32 each is within noise and the plain structure stays)
        const bool w_main = want_wgrad && l == 2 && c->dt != DT_F32 && garena == nullptr;
        auto wgrad_l = [&](hipStream_t st, float* slab) {
            WgradCall g = wgrad_args(c, dvp(l), act(l - 1), G_(di_w(l)), slab, Bd, Ho, Co, Ci);
            g.w.db = G_(di_b(l));                            // bias gradient = column sums of d(pre-activation): rides in the same kernel
            launch_wgrad(g.w, g.max_splits, st);
        };
        if (want_wgrad && !w_main) {
            L.fork(L.a);                                   // d_dv[l] is complete on m here
            wgrad_l(L.a, c->slab);
            if (early_allreduce && l == Ld && c->comm && !c->comm_err && garena == nullptr) {
                // data parallel: the tail of the Discriminator's bucket -- the LAST block's weight (76 % of the bucket) and bias
                // gradient (this kernel, lane a) and the classifier's (k_cls_wgrad, lane b) -- is complete first: its
                // all-reduce starts now, on a lane of its own, under the rest of the backward pass; *_apply reduces the head of
                // the arena and waits for this one (same sums: an all-reduce is elementwise)
                hipEvent_t ea = c->ev_sys[0], eb = c->ev_sys[1];     // (system-scope release: the collective's peers read this arena)
                L.record(ea, L.a); L.record(eb, sb);
                L.wait(c->s_n, ea); L.wait(c->s_n, eb);
                const int64_t o = c->d_off[di_w(l)];
                const int rc = rccl()->AllReduce(ga + o, ga + o, (size_t)(c->d_total - o), NCCL_FLOAT32, NCCL_SUM, c->comm, c->s_n);
                if (rc != NCCL_SUCCESS) L.comm_fail(rc);
                else { L.record(c->ev_ar, c->s_n); early_ar = true; }
            }
        }
        // input gradient ("up" form): contract Cout, produce Cin at (2 Ho x 2 Ho); fused leaky'/dropout of block l-1
        GConvArgs a = gconv_args(c, 1, Bd, Ho, Co, Ci);
        a.in = dvp(l); a.wp = c->d_up[l]; a.out = dvp(l - 1);
        a.epi = EPI_LRELU_BWD; a.aref = act(l - 1); a.noise = nz(l - 1); a.slope = slope;
        launch_gconv(a, L.m);
        if (w_main) {
            L.fork(L.b);                                   // (the first-block reductions start here, beside the weight gradient)
            launch_conv1_wgrad(c->dt, dvp(1), x0, n0, x1, G_(di_w(1)), G_(di_b(1)), c->partial_b, Bd, c->S, c->dC[1], L.b);
            wgrad_l(L.m, c->slab_b);
        }
    }
    if (want_wgrad && c->dt != DT_F32 && garena == nullptr) {
        L.join(L.a);
        L.join(L.b);
    } else if (want_wgrad) {
        // fp32: lane a is still busy with the last (largest-K) weight gradient when the input-gradient chain ends, so the main
        // lane is idle here: block 1's reductions run on it, and the waits for the lanes that ended earlier (lane b, the
        // pipelined Generator forward) are processed in that window too -- every wait is a barrier packet of its own (~5 us
        // each, one after the other), and only the one for lane a is left behind the last kernel
        launch_conv1_wgrad(c->dt, dvp(1), x0, n0, x1, G_(di_w(1)), G_(di_b(1)), c->partial_b, Bd, c->S, c->dC[1], L.m);
        L.join(L.b);
        if (L.tail_wait) L.wait(L.m, L.tail_wait);
        L.join(L.a);
    }
    if (want_dimage)
        launch_conv1_dgrad_tanh(c->dt, dvp(1), c->d_w1t, x0, c->dpre, Bd, c->S, c->dC[1], L.m);
    return early_ar;
}

// Backward through the Generator from d(pre-tanh) in c->dpre; fills the G gradient arena.  Lane m:
// BatchNorm backward and the input-gradient chain; lane a: the weight gradients.
void siggan::g_backward_pass(const siggan_ctx* c, Lanes& L, const float* z, int B) {
    const float gs = c->cfg.g_leaky_slope;                   // the Generator's activation slope (g_dact, act.h)
    const int Lg = c->Lg, S = c->S;
    int pre_rows = 0;              // partial rows of block l's BatchNorm-backward sums left by the input-gradient GEMM of block l+1
    for (int l = Lg; l >= 1; --l) {
        const int Hi = 4 << (l - 1), Ho = 2 * Hi, Ci = c->gC[l - 1], Co = c->gC[l];
        const int64_t R = (int64_t)B * Ho * Ho;
        // dy[l] is complete behind this block's BatchNorm backward: lane a's fork rides on that launch (four marker packets
        // fewer on the lane every kernel of this pass waits on)
        hipEvent_t const ef = L.fork_event(L.a);
        if (l == Lg) {   // final conv's input-gradient folded into this block's BatchNorm backward; its weight gradient rides in
                         // the same pass over y and its row sums stay on this lane (a 5 us kernel does not pay for a fork + join)
            launch_final_bwd_reduce(c->dt, c->dpre, c->wfin_t, c->g_y[l], B, S, Co, c->g_bn[l], c->partial, c->partial_b, gs, L.m);
            launch_final_bn_bwd_apply(c->dt, c->dpre, c->wfin_t, c->g_y[l], c->g_da[l], B, S, Co, c->g_bn[l], c->partial, c->partial_b,
                                      GG(c, gi_fin_w(c)), GG(c, gi_fin_b(c)), GG(c, gi_bn_w(l)), GG(c, gi_bn_b(l)), gs, L.m, ef);
        } else
            launch_bn_bwd(c->dt, c->g_da[l], c->g_y[l], R, Co, c->g_bn[l], c->partial, GG(c, gi_bn_w(l)), GG(c, gi_bn_b(l)), 0, gs, L.m, pre_rows, ef);
        L.fork_after(L.a, ef);
        // weight gradient: small = block input a[l-1] (Hi), large = dy[l] (Ho)
        // (one fork per block; per two blocks measured the same, weight gradients on the main lane 2.5 % slower: DESIGN 4)
        const WgradCall g = wgrad_args(c, c->g_a[l - 1], c->g_da[l], GG(c, gi_up_w(l)), c->slab, B, Hi, Ci, Co);
        launch_wgrad(g.w, g.max_splits, L.a);
        // input gradient ("down" form): out = Cin at Hi, contract Cout over 16 taps
        GConvArgs a = gconv_args(c, 0, B, Ho, Co, Ci);
        a.in = c->g_da[l]; a.wp = c->g_dn[l]; a.out = c->g_da[l - 1]; a.epi = EPI_RAW;
        if (l >= 2) {              // its output is d(activation output) of block l-1: that block's BatchNorm-backward sums ride in the epilogue
            a.epi = EPI_BN_BWD_STATS; a.aref = c->g_y[l - 1]; a.bnp = c->g_bn[l - 1]; a.stat0 = c->partial; a.stat_cap = PARTIAL_FLOATS;
        }
        pre_rows = launch_gconv(a, L.m);
        if (pre_rows < 0) {        // (the pass goes on, so the lanes still join; the step's call returns SIGGAN_E_STATE)
            L.refuse("the Generator's input-gradient GEMM was refused: its BatchNorm-backward sums had no carve (stat_cap)");
            pre_rows = 0;
        }
    }
    if (!(c->fc_fused && launch_fc_bwd_fused(c->dt, c->g_da[0], c->fc_y, z, c->g_bn[0], GG(c, gi_fc_w()), GG(c, gi_fc_b()),
                                             GG(c, gi_bn0_w()), GG(c, gi_bn0_b()), B, c->latent, c->gC[0], gs, L.m))) {
        launch_bn_bwd(c->dt, c->g_da[0], c->fc_y, B, c->F, c->g_bn[0], c->partial, GG(c, gi_bn0_w()), GG(c, gi_bn0_b()),
                      c->gC[0], gs, L.m);
        launch_fc_wgrad(c->dt, c->g_da[0], z, GG(c, gi_fc_w()), GG(c, gi_fc_b()), B, c->latent, c->gC[0], L.m);
    }
    L.join(L.a);
}

// dropout multiplier tables of passes [p0, p1) (pass 0 = rows [0,B) = D(real), pass 1 = rows [B,2B) = D(fake)).
// ctr_add: draw as if the step counter were that much further (a pass generated ahead of its step).
void siggan::make_noise(const siggan_ctx* c, const float* masks, int B, int p0, int p1, hipStream_t s, uint32_t ctr_add) {
    const float keep = 1.0f - c->cfg.dropout;
    int64_t sumC = 0;
    for (int l = 1; l <= c->Ld; ++l) sumC += c->dC[l];
    if (!masks) {
        float* out[8]; int64_t n[8], e0[8]; uint32_t sid[8];
        for (int l = 1; l <= c->Ld; ++l) {
            const int64_t nl = (int64_t)B * c->dC[l];
            out[l - 1] = c->d_noise[l] + p0 * nl; n[l - 1] = nl * (p1 - p0); e0[l - 1] = p0 * nl; sid[l - 1] = 16 + l;
        }
        launch_dropnoise_multi(c->Ld, out, n, e0, sid, keep, c->dev, s, ctr_add);
        return;
    }
    int64_t pre = 0;
    for (int l = 1; l <= c->Ld; ++l) {
        const int64_t n = (int64_t)B * c->dC[l];
        for (int p = p0; p < p1; ++p)
            launch_mask_to_noise(masks + (int64_t)p * B * sumC + (int64_t)B * pre, c->d_noise[l] + p * n, n, keep, s);
        pre += c->dC[l];
    }
}

// The seeds of the per-image objective's backward pass in dpre = d objective / d(pre-tanh image), from the stored fp32 images
// `img` of an eval-mode Generator forward -- shared by the latent calls and siggan_g_param_grad (one sequence, the same bits):
//   [wd > 0]  d_forward_rows at rows [0, B) with stored logits (Ld + 1), the per-image classifier tail k_cls_bwd_eval (1; the
//     realism terms into `realism`, D(G(z)) into probs_dev when given), the Discriminator's input-gradient chain (Ld - 1) and
//     the first block's input-gradient times 1 - x^2 into dpre (1): 2 Ld + 2 launches;
//   [wr > 0]  k_recon_loss (1): the loss partials into partial_b and its seed of dpre -- with wd > 0 added onto the
//     Discriminator's as fmaf(wr, ., dpre).
void siggan::objective_seeds(siggan_ctx* c, const float* img, int B, const uint8_t* target_u8_dev, const float* target_f32_dev,
                            float wr, float wd, float* realism, float* probs_dev, hipStream_t s) {
    const int Ld = c->Ld, S = c->S;
    if (wd > 0.f) {
        c->cs.lP[0] = d_forward_rows(c, img, 0, B, s, c->slab_k);                   // stored logits: siggan_d_forward's bits
        launch_cls_bwd_eval(LogitSrc{c->logits, nullptr, 0, DP(c, di_cls_b(c))}, c->wcp, (const float*)c->d_a[Ld], c->cfg.leaky_slope,
                            (float*)c->d_dv[Ld], B, c->dC[Ld], wd, realism, probs_dev, s);
        for (int l = Ld; l >= 2; --l) {
            GConvArgs a = gconv_args(c, 1, B, S >> l, c->dC[l], c->dC[l - 1]);
            a.in = c->d_dv[l]; a.wp = c->d_up[l]; a.out = c->d_dv[l - 1];
            a.epi = EPI_LRELU_BWD; a.aref = c->d_a[l - 1]; a.noise = nullptr; a.slope = c->cfg.leaky_slope;
            launch_gconv(a, s);
        }
        launch_conv1_dgrad_tanh(c->dt, c->d_dv[1], c->d_w1t, img, c->dpre, B, S, c->dC[1], s);
    }
    if (wr > 0.f)
        launch_recon_loss(img, target_u8_dev, target_f32_dev, c->deq_lut, c->dpre, c->partial_b, B, S, s, wr, wd > 0.f);
}
