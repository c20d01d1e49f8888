// step.hip -- the training step: the four phases (inputs already staged in the workspace: c->real_stage, c->z, c->mask_stage),
// how a phase is enqueued or replayed, and the C ABI's training entry points.  Host code only.
#include "ctx.h"

int siggan::check_hyper(const siggan_hyper* hp) {
    if (!hp) return FAIL(SIGGAN_E_INVALID, "null hyper-parameters");
    if (!(hp->lr >= 0.0) || !(hp->beta1 >= 0.0 && hp->beta1 < 1.0) || !(hp->beta2 >= 0.0 && hp->beta2 < 1.0) || !(hp->eps >= 0.0))
        return FAIL(SIGGAN_E_INVALID, "invalid Adam hyper-parameters");
    return SIGGAN_OK;
}

// D step with a spectrally normalised Discriminator: every training forward runs one power iteration, so the real and the
// fake pass see different effective weights W / sigma_p.  The passes therefore run one after the other on the main lane
// (sigma -> weight packs -> forward), the backward is done per pass with that pass's packs into two arena-shaped
// temporaries, and k_sn_combine forms the gradient w.r.t. weight_orig through both sigmas.
static void phase_d_grads_sn(const siggan_ctx* c, Lanes& L, const PhaseKey& k, PhaseResult& r) {
    const int B = k.B;
    const bool drop = c->cfg.dropout > 0.f;
    repack(c, L, L.m, L.m, k.g_dirty != 0, false);
    if (k.pre_real)
        L.note(hipMemcpyAsync(c->real_stage, k.staged_src, (size_t)B * c->S * c->S * sizeof(float), hipMemcpyDeviceToDevice, L.m));
    if (drop) make_noise(c, k.has_masks ? c->mask_stage : nullptr, B, 0, 2, L.m);
    const float* fake = c->img;
    GFwdOpt ge, gt;                                                  // the eval forward; the G step's training forward
    ge.rng_sid = 1; ge.z_out = c->z; gt.training = true; gt.rng_sid = 2; gt.z_out = c->z_g;
    if (k.variant == SIGGAN_STEP_ABLATION) {
        r.ga_last_B = g_forward_pass(c, k.has_zg ? c->z_g : nullptr, B, c->img_g, L.m, gt);
        L.record(c->ev_gfwd, L.m);
        fake = c->img_g;
    } else {
        r.ga_last_B = g_forward_pass(c, k.has_z ? c->z : nullptr, B, c->img, L.m, ge);
    }
    DFwdOpt fo; fo.dropout = drop;
    launch_sn_sigma(c->snt, 1, 0, SN_EPS, L.m);                       // D(real): power iteration 1
    repack(c, L, L.m, L.m, false, true, 0);
    r.lP[0] = d_forward_rows(c, c->real_stage, 0, B, L.m, c->slab_k, fo);
    launch_sn_sigma(c->snt, 1, 1, SN_EPS, L.m);                       // D(fake): power iteration 2
    repack(c, L, L.m, L.m, false, true, 1);
    r.lP[1] = d_forward_rows(c, fake, B, B, L.m, c->slab_k, fo);
    launch_bce(LogitSrc{c->logits}, 2 * B, B, k.ls, 0.f, c->probs, c->dlogit, k.mt, 0, L.m, c->gscale);     // the step's metrics
    d_backward_pass(c, L, fake, B, fake, B, drop, true, false, BceSpec{B, 0.f, 0.f, nullptr, 0}, r.lP[1], B, c->sn_g[1]);
    repack(c, L, L.m, L.m, false, true, 0);
    d_backward_pass(c, L, c->real_stage, B, c->real_stage, B, drop, true, false, BceSpec{B, k.ls, k.ls, nullptr, 0}, r.lP[0], 0, c->sn_g[0]);
    SnTable t = c->snt;                                               // (a launch-argument table: the slots are this launch's)
    t.slot[0] = 0; t.slot[1] = 1;
    launch_sn_combine(t, c->sn_g[0], c->sn_g[1], c->st.d_grads, c->d_total, 2, L.m);
}

static void phase_d_grads(const siggan_ctx* c, Lanes& L, const PhaseKey& k, PhaseResult& r) {
    r.early_ar = 0;                  // set again by this pass when (and only when) it starts the tail's all-reduce itself
    if (c->sn) return phase_d_grads_sn(c, L, k, r);
    const int B = k.B;
    const bool drop = c->cfg.dropout > 0.f;
    // A staged step whose D(real) forward already ran has nothing for lane a: the real batch is read where it lies (no copy:
    // the borrowed tensor is valid until this call returns), the dropout tables of BOTH passes were drawn when that forward
    // was launched -- no fork, no join, two launches fewer in the step's first 100 us (+0.4 %)
    const bool nolane = k.pre_real == 2 && !k.d_dirty && (!drop || k.dreal_noise2);
    DFwdOpt fo; fo.dropout = drop; fo.fuse_cls = true;
    GFwdOpt ge, gt;                                                  // the eval forward; the G step's training forward
    ge.rng_sid = 1; ge.z_out = c->z; gt.training = true; gt.rng_sid = 2; gt.z_out = c->z_g;
    const float* xreal = c->real_stage;
    int P_real = k.lP0;                                               // (pre_real == 2: as the staged forward left it)
    if (nolane) {
        repack(c, L, L.m, L.m, k.g_dirty != 0, false);
        xreal = k.staged_src;
    } else {
    L.fork(L.a);                                                     // lane a: D's packs, dropout tables, D(real)
    repack(c, L, L.m, L.a, k.g_dirty != 0, k.d_dirty != 0);
    if (k.pre_real)      // staged batch -> this step's real batch (the D backward reads it again)
        L.note(hipMemcpyAsync(c->real_stage, k.staged_src, (size_t)B * c->S * c->S * sizeof(float), hipMemcpyDeviceToDevice, L.a));
    if (drop && !(k.pre_real == 2 && k.dreal_noise2))
        make_noise(c, k.has_masks ? c->mask_stage : nullptr, B, k.pre_real == 2 ? 1 : 0, 2, L.a);
    // D(real) beside the Generator (train...py:309) -- unless the previous siggan_g_grads already ran it
    // (siggan_stage_real) beside its Generator backward; then bce only has to wait for that lane
    if (k.pre_real != 2) r.lP[0] = P_real = d_forward_rows(c, c->real_stage, 0, B, L.a, c->slab_k2, fo);
    }
    const float* fake = c->img;
    const bool spec_fwd = k.spec_g && k.variant != SIGGAN_STEP_ABLATION;
    // siggan_step_begin: the G step's training forward depends on nothing the D step changes.  16-bit contexts (every kernel
    // is a few microseconds: the step is a chain of launch latencies) start it HERE, beside the eval forward, with the eval
    // forward's activations in buffers of their own: bf16 batch 64 0.747 -> 0.723 ms.  fp32 keeps it behind D(fake) (below):
    // there the early start measured 0.7 % slower (round 3) / 0.1 % faster with fence-free events (round 4: noise) -- its
    // BatchNorm / fc kernels take matrix-pipe time from the eval forward, which is on the step's critical lane.
    const bool spec_early = spec_fwd && c->dt != DT_F32;
    hipEvent_t e_early = nullptr, e_eval = nullptr;
    if (spec_early) { e_early = L.next(); L.record(e_early, L.m); }
    if (k.variant == SIGGAN_STEP_ABLATION) {
        // ablation_vanilla_gan_signatures.py:397-448: both nets in train mode and ONE Generator forward per iteration --
        // BatchNorm batch statistics (+ running update), activations kept: the D half sees fake.detach(), the G half
        // back-propagates through the very same forward
        r.ga_last_B = g_forward_pass(c, k.has_zg ? c->z_g : nullptr, B, c->img_g, L.m, gt);
        L.record(c->ev_gfwd, L.m);
        fake = c->img_g;
    } else {
        // (nolane: the pipelined forward below needs nothing but this pass -- its fork rides on the last kernel here)
        if (spec_fwd && !spec_early && nolane) e_eval = L.fork_event(c->s_c);
        ge.done = e_eval;
        r.ga_last_B = g_forward_pass(c, k.has_z ? c->z : nullptr, B, c->img, L.m, ge);   // G.eval(), no grad (train...py:314-315)
    }
    if (spec_early) {       // (enqueued behind the eval forward: the critical lane's kernels reach the dispatcher first)
        L.wait(c->s_c, e_early);
        gt.partial = c->partial_c; gt.slab_k = c->slab_k3;
        r.ga_last_B = g_forward_pass(c, k.has_zg ? c->z_g : nullptr, B, c->img_g, c->s_c, gt);
        L.record(c->ev_gfwd, c->s_c);
    }
    if (!nolane) L.join(L.a);
    // siggan_step_begin: the G step's training forward depends on nothing the D step changes, so it
    // runs on its own lane beside D(fake) and the D step's backward (after the eval forward above: it
    // moves the BatchNorm running statistics and reuses the activation buffers; its own image / z /
    // scratch).  It forks HERE but is enqueued after D(fake), whose kernels the dispatcher should see first.
    hipEvent_t e_spec = nullptr;
    if (spec_fwd && !spec_early) { e_spec = e_eval; if (!e_spec) { e_spec = L.next(); L.record(e_spec, L.m); } }
    // the staged D(real) launch (lane c, previous G step) also drew THIS pass' dropout tables (dreal_noise2): the main lane
    // must be behind that lane before D(fake) reads them, not only before the backward pass reads the rows
    const bool join_early = k.pre_real == 2 && !k.dreal_joined && drop && k.dreal_noise2;
    if (join_early) L.wait(L.m, c->ev_dreal);
    r.lP[1] = d_forward_rows(c, fake, B, B, L.m, c->slab_k, fo);   // D(fake) into rows [B, 2B)
    if (k.pre_real == 2 && !k.dreal_joined && !join_early) L.wait(L.m, c->ev_dreal);
    r.dreal_joined = r.dreal_noise2 = 0;
    if (spec_fwd && !spec_early) {
        L.wait(c->s_c, e_spec);
        gt.partial = c->partial_c; gt.slab_k = c->slab_k2;
        r.ga_last_B = g_forward_pass(c, k.has_zg ? c->z_g : nullptr, B, c->img_g, c->s_c, gt);
        L.record(c->ev_gfwd, c->s_c);
    }
    // the pipelined forward has ended by the time the weight gradients have: the main lane waits for it inside the backward
    // pass' tail (fp32) / next to the two joins of this phase (16-bit), not between the optimiser and the G step's first kernel
    if (spec_fwd && c->dt == DT_F32) L.tail_wait = c->ev_gfwd;
    r.early_ar = d_backward_pass(c, L, xreal, B, fake, 2 * B, drop, true, false, BceSpec{B, k.ls, 0.f, k.mt, 0},
                                 P_real == r.lP[1] ? P_real : -1, 0, nullptr, k.coll != 0);
    L.tail_wait = nullptr;
    if (spec_fwd && c->dt != DT_F32) L.wait(L.m, c->ev_gfwd);
    r.gfwd_joined = spec_fwd;
}

static void phase_g_grads(const siggan_ctx* c, Lanes& L, const PhaseKey& k, PhaseResult& r) {
    const int B = k.B;
    const float* zg; float* img;
    const bool d_pack = !c->sn && k.d_dirty != 0;                    // (spectral norm: the packs follow sigma, below)
    bool conv1_done = false;
    if (k.spec_g) {                                                  // forward already enqueued by siggan_step_begin
        if (!k.gfwd_joined) L.wait(L.m, c->ev_gfwd);
        r.gfwd_joined = 0;
        // trainer step: the first-block forward of the new images (rows [B, 2B), no dropout in this pass) rides in the launch
        // that re-packs D's weights -- it reads the raw block-1 weights, and the two would stand back to back on this lane
        // (k.rode: both already happened in the D update's launch, k_adam_pack)
        conv1_done = k.rode || (d_pack && k.variant != SIGGAN_STEP_ABLATION);
        repack(c, L, L.m, L.m, false, d_pack, 0, (conv1_done && !k.rode) ? c->img_g : nullptr, B, B);
        zg = c->z_g; img = c->img_g;
    } else {
        L.fork(L.a);
        repack(c, L, L.m, L.a, k.g_dirty != 0, d_pack);
        GFwdOpt gt; gt.training = true; gt.rng_sid = 2; gt.z_out = c->z;
        r.ga_last_B = g_forward_pass(c, k.has_z ? c->z : nullptr, B, c->img, L.m, gt);   // G.train(): BN batch stats (train...py:349)
        L.join(L.a);
        zg = c->z; img = c->img;
    }
    // trainer step: D.eval() -- dropout off, target 1.0 (train...py:350,360).  Ablation step: D stays in train mode -- a
    // fresh set of dropout masks -- and the target is the smoothed real label (ablation...py:441-442)
    const bool abl = k.variant == SIGGAN_STEP_ABLATION;
    const bool gdrop = abl && c->cfg.dropout > 0.f;
    if (c->sn) {        // D.eval() (trainer step): sigma from the stored u, v; D.train() (ablation step): a third power iteration
        launch_sn_sigma(c->snt, abl ? 1 : 0, 2, SN_EPS, L.m);
        repack(c, L, L.m, L.m, false, true, 2);
    }
    if (gdrop) {
        int64_t sumC = 0;
        for (int l = 1; l <= c->Ld; ++l) sumC += c->dC[l];
        make_noise(c, k.has_masks ? c->mask_stage + (int64_t)2 * B * sumC : nullptr, B, 0, 1, L.m);
    }
    const float gy = abl ? k.ls : 1.0f;
    // The G step's Discriminator pass runs in workspace rows [B, 2B) -- free since the D step's backward -- so that the NEXT D
    // step's D(real) forward (rows [0, B), siggan_stage_real) can start right here, beside this pass's forward and
    // input-gradient chain (one B-sized GEMM at a time leaves half the chip's wave slots idle), not only beside the Generator
    // backward: +1.3 % (round 3).  (ablation step: its dropout tables are drawn for rows [0, B); spectral norm: no staging)
    const int r0g = (!abl && !c->sn) ? B : 0;
    r.g_r0 = r0g;
    const bool real_early = k.pre_real && r0g != 0;
    if (real_early) {
        const bool drop = c->cfg.dropout > 0.f;
        L.fork(c->s_c);                                               // D's packs are complete on m here
        if (drop) make_noise(c, nullptr, B, 0, 2, c->s_c, 1);       // the D(fake) pass' tables too (this G step's pass has no dropout)
        r.dreal_noise2 = drop;
        DFwdOpt ro; ro.dropout = drop; ro.fuse_cls = true;
        r.lP[0] = d_forward_rows(c, k.staged_src, 0, B, c->s_c, c->slab_k2, ro);
        L.record(c->ev_dreal, c->s_c);
    }
    DFwdOpt fo; fo.dropout = gdrop; fo.fuse_cls = true; fo.conv1_done = conv1_done;
    const int P = r.lP[r0g ? 1 : 0] = d_forward_rows(c, img, r0g, B, L.m, c->slab_k, fo);
    d_backward_pass(c, L, img, B, img, B, gdrop, false, true, BceSpec{B, gy, gy, k.mt, 1}, P, r0g);   // through D into the image; no D weight grads
    if (k.pre_real && !real_early) {
        // siggan_stage_real: the NEXT D step's D(real) forward needs the Discriminator as it is now (its
        // update is behind us) and the activation rows this step is done with: run it on lane c beside the
        // Generator backward.  Its dropout tables are drawn for the step counter that step will see (+1:
        // the Generator update in between ticks once).
        const bool drop = c->cfg.dropout > 0.f;
        L.fork(c->s_c);
        if (drop) make_noise(c, nullptr, B, 0, 1, c->s_c, 1);
        DFwdOpt ro; ro.dropout = drop; ro.fuse_cls = true;
        r.lP[0] = d_forward_rows(c, k.staged_src, 0, B, c->s_c, c->slab_k2, ro);
        L.record(c->ev_dreal, c->s_c);
    }
    g_backward_pass(c, L, zg, B);
    // 16-bit contexts: join the early D(real) lane HERE, next to the join of the weight-gradient lane, so that the next D step
    // does not stop for it behind D(fake)
    if (real_early && c->dt != DT_F32) { L.wait(L.m, c->ev_dreal); r.dreal_joined = 1; }
}

// one network's optimiser state (which: 0 G, 1 D): its arenas, their size and tensor count, its two metric slots
struct Net { float *p, *g, *m, *v, *steps; int64_t n; int nt, m_norm, m_skipped; };
static Net net_of(const siggan_ctx* c, int which) {
    const siggan_storage& s = c->st;
    if (which == 0) return {s.g_params, s.g_grads, s.g_exp_avg, s.g_exp_avg_sq, s.g_adam_steps, c->g_total, (int)c->g_off.size(),
                            SIGGAN_M_G_GRAD_NORM, SIGGAN_M_G_SKIPPED};
    return {s.d_params, s.d_grads, s.d_exp_avg, s.d_exp_avg_sq, s.d_adam_steps, c->d_total, (int)c->d_off.size(),
            SIGGAN_M_D_GRAD_NORM, SIGGAN_M_D_SKIPPED};
}

static void phase_apply(const siggan_ctx* c, Lanes& L, const PhaseKey& k, PhaseResult& r) {
    const int which = k.phase == 2 ? 1 : 0;                          // phase 2 = D apply, 3 = G apply
    const Net N = net_of(c, which);
    float* const g = N.g;
    float *const mt_norm = k.mt + N.m_norm, *const mt_skipped = k.mt + N.m_skipped;
    const bool clip = k.clip > 0.f;
    // the arena holds gscale x the gradient (fp16 chains; 1 otherwise): the optimiser's multiplier takes it out again, and
    // the gradient is written back unscaled (as torch leaves a clipped .grad)
    float gs = k.gs / c->gscale;
    if (c->comm) {
        // the data-parallel exchange: ONE sum all-reduce of the network's flat gradient bucket over RCCL, in place, on the
        // step's own stream (whatever runs on the side lanes -- the pipelined Generator forward behind the D bucket, the
        // staged D(real) forward behind the G bucket -- overlaps it); the mean is taken by the optimiser's multiplier
        // a failed (or earlier failed) exchange leaves this rank's arena unreduced: the optimiser must not step on it --
        // the update is skipped and lane_check hands the error to the caller (sticky: every later call returns it until
        // siggan_comm_destroy)
        if (c->comm_err) return;
        if (which == 1 && k.early_ar) {
            // the tail of the arena (last block + classifier) went ahead (d_backward_pass): the head now
            const int64_t o = c->d_off[di_w(c->Ld)];
            const int e = rccl()->AllReduce(g, g, (size_t)o, NCCL_FLOAT32, NCCL_SUM, c->comm, L.m);
            r.early_ar = 0;
            if (e != NCCL_SUCCESS) { L.comm_fail(e); return; }
            L.wait(L.m, c->ev_ar);
        } else {
        const int e = rccl()->AllReduce(g, g, (size_t)N.n, NCCL_FLOAT32, NCCL_SUM, c->comm, L.m);
        if (e != NCCL_SUCCESS) { L.comm_fail(e); return; }
        }
        gs *= 1.0f / (float)c->comm_world;
    }
    const bool guard = c->dt == DT_F16;                              // static gradient scale: skip the update on an overflow
    if (clip || guard) launch_grad_sumsq(g, N.n, c->partial, L.m);
    if (k.fused_t > 0.0 && k.pack) {
        // ... and the same launch rebuilds what the next pass derives from the arena (weight packs, eval tables): no
        // k_prepare between the update and the forward pass that follows it on the step's critical lane
        ApTable t;
        ApRide rd; memset(&rd, 0, sizeof rd);
        if (k.ride) {      // the pending G step's first Discriminator block (siggan_step_begin's images; rows [B, 2B)) rides along
            if (!k.gfwd_joined) { L.wait(L.m, c->ev_gfwd); r.gfwd_joined = 1; }
            const int64_t H = c->S >> 1;
            rd.x = c->img_g; rd.out = c->d_a[1] + (size_t)((int64_t)k.ride * H * H * c->dC[1]) * c->es; rd.B = k.ride; rd.S = c->S;
            rd.dt = c->dt; rd.slope = c->cfg.leaky_slope; rd.w_off = c->d_off[di_w(1)]; rd.b_off = c->d_off[di_b(1)];
            rd.counter = (unsigned*)c->ride_ctr; rd.late = c->ride_late_dev;
        }
        ap_table(c, which, k.ride * (c->S / 4), t);
        if (!launch_adam_pack(t, N.p, g, N.m, N.v, c->dev, N.steps, N.nt, k.fused_t, k.lr, k.beta1, k.beta2, k.eps, gs, k.clip, mt_norm,
                              clip ? c->partial : nullptr, mt_skipped, BN_EPS, k.ride ? &rd : nullptr, L.m))
            L.note(hipErrorInvalidValue);                               // (table overflow: not reached)
        return;
    }
    if (k.fused_t > 0.0) {
        // ONE launch: the host knows the step count (apply_common), so the bias corrections are kernel arguments and
        // k_adam_prepare (a 5 us kernel plus a kernel boundary on the step's critical lane, twice per step) is not needed
        launch_adam_fused(N.p, g, N.m, N.v, N.n, c->dev, N.steps, N.nt, k.fused_t, k.lr, k.beta1, k.beta2, k.eps, gs, k.clip, mt_norm,
                          clip ? c->partial : nullptr, L.m, mt_skipped);
        return;
    }
    launch_adam_prepare(c->dev, N.steps, N.nt, k.lr, k.beta1, k.beta2, gs, k.clip, mt_norm, L.m, guard ? 1 : 0, mt_skipped,
                        (clip || guard) ? c->partial : nullptr);
    launch_adam(N.p, g, N.m, N.v, N.n, c->dev, k.beta1, k.beta2, k.eps, (clip || gs != 1.0f) ? 1 : 0, L.m);
}

static PhaseResult run_phase_body(const siggan_ctx* c, Lanes& L, const PhaseKey& k) {
    PhaseResult r;
    if (k.phase == 0) phase_d_grads(c, L, k, r);
    else if (k.phase == 1) phase_g_grads(c, L, k, r);
    else phase_apply(c, L, k, r);
    return r;
}

// Enqueue one phase behind everything on the caller's stream u.  Eager: directly on u (side lanes
// forked from it).  Graph mode: the phase is captured once per distinct key on the library's own
// main lane (a caller stream may be the legacy default stream, which cannot be captured) and replayed.
// r: what the phase leaves behind -- of the enqueue just made, or (replay) of the capture, kept beside the graph.
static int enqueue_phase(siggan_ctx* c, const PhaseKey& k, hipStream_t u, PhaseResult& r) {
    if (c->refused) return lane_check(c);           // a step's launch was refused: nothing more is enqueued on this context
    const bool overlap = (c->mode & SIGGAN_MODE_OVERLAP) != 0;
    const bool graph = (c->mode & SIGGAN_MODE_GRAPH) != 0 && g_prof == nullptr;
    if (graph && c->comm && k.phase >= 2) return FAIL(SIGGAN_E_STATE, "SIGGAN_MODE_GRAPH is not available with a communicator");
    if (graph && c->sn) return FAIL(SIGGAN_E_STATE, "SIGGAN_MODE_GRAPH is not available with spectral normalisation");
    if (!graph) {
        const bool ext = overlap && g_prof == nullptr;
        Lanes L(c, u, overlap ? c->s_a : u, overlap ? c->s_b : u, ext);
        r = run_phase_body(c, L, k);
        LAUNCHCHK();
        return lane_check(c);
    }
    hipGraphExec_t exec = nullptr;
    for (auto& e : c->graphs)
        if (e.key == k) { exec = e.exec; r = e.res; break; }
    if (!exec) {
        Lanes L(c, c->s_m, overlap ? c->s_a : c->s_m, overlap ? c->s_b : c->s_m, false);
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(c->s_m, hipStreamCaptureModeRelaxed));
        r = run_phase_body(c, L, k);
        hipError_t e1 = hipStreamEndCapture(c->s_m, &g);
        if (e1 != hipSuccess || !g) return FAIL(SIGGAN_E_HIP, "stream capture failed: %s", hipGetErrorString(e1));
        if (c->refused) { (void)hipGraphDestroy(g); return lane_check(c); }     // (a refused launch: not cached, never replayed)
        hipError_t e2 = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e2 != hipSuccess) return FAIL(SIGGAN_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e2));
        if (c->graphs.size() >= 64) { (void)hipGraphExecDestroy(c->graphs.front().exec); c->graphs.erase(c->graphs.begin()); }
        c->graphs.push_back(CachedPhase{k, exec, r});
    }
    hipEvent_t e_in = c->ev_bridge[0], e_out = c->ev_bridge[1];
    HIPCHK(hipEventRecord(e_in, u));
    HIPCHK(hipStreamWaitEvent(c->s_m, e_in, 0));
    HIPCHK(hipGraphLaunch(exec, c->s_m));
    HIPCHK(hipEventRecord(e_out, c->s_m));
    HIPCHK(hipStreamWaitEvent(u, e_out, 0));
    return SIGGAN_OK;
}
static int run_phase(siggan_ctx* c, const PhaseKey& k, hipStream_t u) {
    PhaseResult r;
    const int rc = enqueue_phase(c, k, u, r);
    // the ONE place a phase's results reach the context (also when a check after the enqueue failed: the work is in flight)
    Carried& cs = c->cs;
    auto put = [](auto& field, int v) { if (v >= 0) field = v; };
    put(cs.early_ar, r.early_ar); put(cs.dreal_joined, r.dreal_joined); put(cs.dreal_noise2, r.dreal_noise2);
    put(cs.gfwd_joined, r.gfwd_joined); put(cs.g_r0, r.g_r0); put(cs.ga_last_B, r.ga_last_B);
    put(cs.lP[0], r.lP[0]); put(cs.lP[1], r.lP[1]);
    return rc;
}

static PhaseKey make_key(siggan_ctx* c, int phase, int B, bool has_z, bool has_masks, const siggan_hyper* hp,
                         float* metrics_dev) {
    PhaseKey k; memset(&k, 0, sizeof k);
    k.phase = phase; k.B = B; k.has_z = has_z; k.has_masks = has_masks;
    k.mt = metrics_dev ? metrics_dev : c->metrics;
    if (phase <= 1) { k.g_dirty = c->g_dirty; k.d_dirty = c->d_dirty; k.ls = hp->label_smoothing; }
    else {
        k.lr = hp->lr; k.beta1 = hp->beta1; k.beta2 = hp->beta2; k.eps = hp->eps;
        k.clip = hp->clip_max_norm > 0.f ? hp->clip_max_norm : 0.f;
        k.gs = hp->grad_scale > 0.f ? hp->grad_scale : 1.0f;
    }
    return k;
}

static int finish_metrics(siggan_ctx* c, float* metrics_dev, float* metrics_host, hipStream_t s) {
    if (metrics_host) {
        HIPCHK(hipMemcpyAsync(metrics_host, metrics_dev ? metrics_dev : c->metrics, SIGGAN_M_COUNT * sizeof(float),
                              hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return SIGGAN_OK;
}

static int d_grads_common(siggan_ctx* c, const float* real_dev, int32_t batch, const float* z_dev, const float* masks_dev,
                          const siggan_hyper* hp, float* metrics_dev, void* stream, bool spec_g, const float* zg_dev,
                          bool apply_follows = false) {
    ENTER(c);
    Carried& cs = c->cs;
    int rc = check_call(c, batch);
    if (rc) return rc;
    if ((rc = check_hyper(hp))) return rc;
    if (!real_dev && cs.staged_B != batch)
        return FAIL(SIGGAN_E_INVALID, "null real batch (and no batch of %d images staged by siggan_stage_real)", batch);
    if (!c->st.d_grads) return FAIL(SIGGAN_E_STATE, "gradient arena was not bound");
    if (cs.g_fwd_pending) return FAIL(SIGGAN_E_STATE, "siggan_step_begin must be followed by siggan_g_grads before the next D step");
    // the speculative forward needs its own lane: without overlap (or under graph replay) it is skipped
    if (spec_g && ((c->mode & SIGGAN_MODE_OVERLAP) == 0 || (c->mode & SIGGAN_MODE_GRAPH) != 0 || g_prof != nullptr)) spec_g = false;
    const bool abl = c->variant == SIGGAN_STEP_ABLATION;
    // spectral norm, trainer step: phase_d_grads_sn runs its passes one after the other on the main lane and has no
    // pipelined Generator forward -- siggan_g_grads then runs the training forward itself (an explicit zg_dev waits in
    // z_g, zg_stash)
    if (c->sn && !abl) spec_g = false;
    // one sample: the reference's D step runs (G.eval()) and its G step then refuses the batch -- no forward ahead of that
    if (batch == 1 && !abl) spec_g = false;
    if (abl) {                                 // one z per iteration: it belongs to the (single, training-mode) Generator forward
        if ((rc = check_bn_batch(c, batch))) return rc;
        if (zg_dev) return FAIL(SIGGAN_E_INVALID, "the ablation step has one latent batch per iteration: pass it as z_dev");
        zg_dev = z_dev; z_dev = nullptr; spec_g = true;
    }
    hipStream_t s = (hipStream_t)stream;
    const int B = batch;
    const size_t img_bytes = (size_t)B * c->S * c->S * sizeof(float);
    // stage the caller's tensors into fixed workspace slots (captured phases must see fixed addresses)
    int pre_real = 0;                          // 1: the staged batch is this step's real batch; 2: and its D(real) forward is done
    if (!real_dev) pre_real = (cs.dreal_B == B && !masks_dev) ? 2 : 1;
    if (pre_real == 2) cs.dreal_B = 0;         // consumed: the phase waits for ev_dreal where it needs the rows
    else drop_dreal(c);                        // D(real) is redone (explicit batch / masks): the early one is abandoned
    if ((rc = settle(c, s))) return rc;
    if (real_dev && real_dev != c->real_stage) HIPCHK(hipMemcpyAsync(c->real_stage, real_dev, img_bytes, hipMemcpyDeviceToDevice, s));
    cs.staged_B = 0;
    if (z_dev && z_dev != c->z) HIPCHK(hipMemcpyAsync(c->z, z_dev, (size_t)B * c->latent * sizeof(float), hipMemcpyDeviceToDevice, s));
    int64_t sumC = 0;
    for (int l = 1; l <= c->Ld; ++l) sumC += c->dC[l];
    if (masks_dev) HIPCHK(hipMemcpyAsync(c->mask_stage, masks_dev, (size_t)(abl ? 3 : 2) * B * sumC * sizeof(float), hipMemcpyDeviceToDevice, s));
    cs.abl_masks = abl && masks_dev != nullptr;
    if (zg_dev) HIPCHK(hipMemcpyAsync(c->z_g, zg_dev, (size_t)B * c->latent * sizeof(float), hipMemcpyDeviceToDevice, s));
    cs.zg_stash = (!spec_g && zg_dev) ? B : 0;
    PhaseKey k = make_key(c, 0, B, z_dev != nullptr, masks_dev != nullptr, hp, metrics_dev);
    cs.metrics_last = k.mt;
    k.spec_g = spec_g; k.has_zg = spec_g && zg_dev != nullptr; k.pre_real = pre_real; k.variant = c->variant;
    if (pre_real) k.staged_src = cs.staged_src;
    if (pre_real == 2) { k.dreal_joined = cs.dreal_joined; k.dreal_noise2 = cs.dreal_noise2; k.lP0 = cs.lP[0]; }
    k.coll = apply_follows && c->comm != nullptr && (c->mode & SIGGAN_MODE_GRAPH) == 0;   // (no collective inside a captured phase)
    if ((rc = run_phase(c, k, s))) return rc;
    c->g_dirty = c->d_dirty = false;
    if (spec_g) { cs.g_fwd_pending = B; c->g_dirty = true; }   // running statistics moved
    cs.pending = 1;
    return SIGGAN_OK;
}

extern "C" int siggan_stage_real(siggan_ctx* c, const float* real_dev, int32_t batch, void* stream) {
    ENTER(c);
    int rc = check_call(c, batch);
    if (rc) return rc;
    if (!real_dev) return FAIL(SIGGAN_E_INVALID, "null real batch");
    invalidate(c, INV_STREAM);         // an early D(real) forward of a previously staged batch may still be reading that batch
    if ((rc = settle(c, (hipStream_t)stream))) return rc;
    // borrowed, not copied (a 1 MB copy on the step's critical lane): the caller keeps the tensor alive and unmodified until the
    // D step that consumes it has returned (include/siggan.h); that step copies it into the workspace on a side lane
    c->cs.staged_src = real_dev;
    c->cs.staged_B = batch;
    return SIGGAN_OK;
}

extern "C" int siggan_d_grads(siggan_ctx* c, const float* real_dev, int32_t batch, const float* z_dev, const float* masks_dev,
                              const siggan_hyper* hp, float* metrics_dev, void* stream) {
    return d_grads_common(c, real_dev, batch, z_dev, masks_dev, hp, metrics_dev, stream, false, nullptr);
}

extern "C" int siggan_step_begin(siggan_ctx* c, const float* real_dev, int32_t batch, const float* z_dev, const float* masks_dev,
                                 const float* zg_dev, const siggan_hyper* hp, float* metrics_dev, void* stream) {
    return d_grads_common(c, real_dev, batch, z_dev, masks_dev, hp, metrics_dev, stream, true, zg_dev, true);
}

static int apply_common(siggan_ctx* c, int which, const siggan_hyper* hp, float* metrics_dev, float* metrics_host, void* stream) {
    ENTER(c);
    Carried& cs = c->cs;
    int rc = check_call(c, 1);
    if (rc) return rc;
    if ((rc = check_hyper(hp))) return rc;
    if (cs.pending != (which == 1 ? 1 : 2))
        return FAIL(SIGGAN_E_STATE, "siggan_%c_apply without a preceding siggan_%c_grads", which ? 'd' : 'g', which ? 'd' : 'g');
    const Net N = net_of(c, which);
    for (const float* p : {N.g, N.m, N.v, N.steps})
        if (!p) return FAIL(SIGGAN_E_STATE, "gradient / Adam arenas were not bound");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = settle(c, s))) return rc;
    // metrics of a step live in ONE buffer: the one the *_grads call named (its losses are already there)
    if (!metrics_dev) metrics_dev = cs.metrics_last != c->metrics ? cs.metrics_last : nullptr;
    else if (cs.metrics_last && metrics_dev != cs.metrics_last)
        HIPCHK(hipMemcpyAsync(metrics_dev, cs.metrics_last, SIGGAN_M_COUNT * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    PhaseKey k = make_key(c, which == 1 ? 2 : 3, 0, false, false, hp, metrics_dev);
    if (which == 1) k.early_ar = cs.early_ar;
    // One-launch update whenever the step count can live on the host: not under graph replay (arguments are baked into the
    // captured launch) and not with the fp16 overflow guard (a skipped update leaves the device-side count behind).  The count
    // is read back once after siggan_bind / siggan_params_changed and tracked from then on.
    const int wi = which == 1 ? 1 : 0;
    if ((c->mode & SIGGAN_MODE_GRAPH) == 0 && c->dt != DT_F16) {
        if (!c->adam_t_known[wi]) {
            float t0 = 0.f;
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy(&t0, N.steps, sizeof t0, hipMemcpyDeviceToHost));
            c->adam_t[wi] = (double)t0; c->adam_t_known[wi] = true;
        }
        k.fused_t = c->adam_t[wi] + 1.0;
        k.pack = c->packable[which] ? 1 : 0;
        // trainer step with the G step's training forward already enqueued (siggan_step_begin): its first Discriminator block
        // needs nothing but the updated block-1 weights -- it rides in the update's launch (phase_g_grads then skips it).
        // fp32 only: 1.4201 -> 1.4105 ms; at bf16 the separate launch measured better (0.6216 vs 0.6245 ms)
        if (which == 1 && k.pack && cs.g_fwd_pending && c->variant != SIGGAN_STEP_ABLATION && g_prof == nullptr && c->dt == DT_F32) {
            k.ride = cs.g_fwd_pending; k.gfwd_joined = cs.gfwd_joined;
        }
    } else {
        c->adam_t_known[wi] = false;
    }
    if ((rc = run_phase(c, k, s))) return rc;
    if (k.fused_t > 0.0) c->adam_t[wi] = k.fused_t;
    // (k.pack: the launch that updated the arena also rebuilt what is derived from it, with the running statistics as the
    // G step's training forward left them)
    if (which == 0) c->g_dirty = !k.pack; else c->d_dirty = !k.pack;
    if (which == 1) cs.conv1_rode = k.ride;
    cs.pending = 0;
    return finish_metrics(c, metrics_dev, metrics_host, s);
}

extern "C" int siggan_d_apply(siggan_ctx* c, const siggan_hyper* hp, float* metrics_dev, float* metrics_host, void* stream) {
    return apply_common(c, 1, hp, metrics_dev, metrics_host, stream);
}

extern "C" int siggan_d_step(siggan_ctx* c, const float* real_dev, int32_t batch, const float* z_dev, const float* masks_dev,
                             const siggan_hyper* hp, float* metrics_dev, float* metrics_host, void* stream) {
    int rc = d_grads_common(c, real_dev, batch, z_dev, masks_dev, hp, metrics_dev, stream, false, nullptr, true);
    if (rc) return rc;
    return siggan_d_apply(c, hp, metrics_dev, metrics_host, stream);
}

extern "C" int siggan_g_grads(siggan_ctx* c, int32_t batch, const float* z_dev, const siggan_hyper* hp, float* metrics_dev,
                              void* stream) {
    ENTER(c);
    Carried& cs = c->cs;
    int rc = check_call(c, batch);
    if (rc) return rc;
    if ((rc = check_bn_batch(c, batch))) return rc;
    if ((rc = check_hyper(hp))) return rc;
    if (!c->st.g_grads) return FAIL(SIGGAN_E_STATE, "gradient arena was not bound");
    hipStream_t s = (hipStream_t)stream;
    if ((rc = settle(c, s))) return rc;
    const int B = batch;
    const bool spec = cs.g_fwd_pending != 0;
    if (c->variant == SIGGAN_STEP_ABLATION && !spec)
        return FAIL(SIGGAN_E_STATE, "ablation step: siggan_g_grads follows the siggan_d_grads / siggan_d_apply of the same iteration");
    if (spec && (cs.g_fwd_pending != B || z_dev))
        return FAIL(SIGGAN_E_STATE, "siggan_g_grads after siggan_step_begin must use the same batch and no explicit z (pass it to step_begin)");
    if (!spec && !z_dev && cs.zg_stash == B) z_dev = c->z_g;          // z given to a step_begin that could not pipeline
    cs.zg_stash = 0;
    if (!spec && z_dev && z_dev != c->z) HIPCHK(hipMemcpyAsync(c->z, z_dev, (size_t)B * c->latent * sizeof(float), hipMemcpyDeviceToDevice, s));
    PhaseKey k = make_key(c, 1, B, z_dev != nullptr, false, hp, metrics_dev);
    cs.metrics_last = k.mt;
    k.spec_g = spec; k.variant = c->variant; k.has_masks = cs.abl_masks;
    if (spec) k.gfwd_joined = cs.gfwd_joined;
    k.rode = (spec && cs.conv1_rode == B && !c->d_dirty) ? 1 : 0;
    cs.conv1_rode = 0;
    cs.abl_masks = false;
    // a staged next batch: start its D(real) forward beside this Generator backward (own lane: eager overlap mode only)
    k.pre_real = cs.staged_B == B && cs.dreal_B == 0 && (c->mode & SIGGAN_MODE_OVERLAP) != 0 && (c->mode & SIGGAN_MODE_GRAPH) == 0 &&
                 g_prof == nullptr && cs.pending == 0 && !c->sn;
    if (k.pre_real) k.staged_src = cs.staged_src;
    if ((rc = run_phase(c, k, s))) return rc;
    cs.g_rode = k.rode ? B : 0; cs.g_pre_real = k.pre_real ? B : 0;
    if (k.pre_real) cs.dreal_B = B;
    cs.g_fwd_pending = 0;
    c->d_dirty = false;
    c->g_dirty = true;                 // the training forward moved the BatchNorm running statistics
    cs.pending = 2;
    return SIGGAN_OK;
}

extern "C" int siggan_g_apply(siggan_ctx* c, const siggan_hyper* hp, float* metrics_dev, float* metrics_host, void* stream) {
    return apply_common(c, 0, hp, metrics_dev, metrics_host, stream);
}

extern "C" int siggan_g_step(siggan_ctx* c, int32_t batch, const float* z_dev, const siggan_hyper* hp, float* metrics_dev,
                             float* metrics_host, void* stream) {
    int rc = siggan_g_grads(c, batch, z_dev, hp, metrics_dev, stream);
    if (rc) return rc;
    return siggan_g_apply(c, hp, metrics_dev, metrics_host, stream);
}
