// siggan.hip -- C ABI (include/siggan.h) of the MI355X signature-GAN engine: the context's lifecycle, layout and queries.  The
// passes: passes.hip; the training step: step.hip; the other entry points: eval.hip, extras.hip; what they share: ctx.h.
//
// One context = one GPU.  The caller (PyTorch-ROCm tensors, through ctypes) owns parameters,
// gradients, Adam moments and BatchNorm buffers as flat fp32 arenas in the reference's
// parameters() order; the library owns only the workspace allocated here (NHWC activations,
// packed weight copies, split-K slabs, reduction partials, device-side step state).
#include "ctx.h"

static thread_local char g_err[512] = "";
// (every file reports through this one thread-local message: FAIL, host.h)
int siggan_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int siggan_abi_version(void) { return SIGGAN_ABI_VERSION; }
extern "C" const char* siggan_last_error(void) { return g_err; }

static void build_layout(siggan_ctx* c) {
    // (the chains, and slab_k_floats below: restated in tests/evalpaths.py, matched as text by tests/test_eval_paths_cpu.py)
    static const int g64[] = {256, 128, 64, 32, 32}, g128[] = {512, 256, 128, 64, 32, 32};
    static const int d64[] = {1, 64, 128, 256, 512}, d128[] = {1, 64, 128, 256, 512, 512};
    if (c->S == 64) { c->Lg = 4; c->Ld = 4; memcpy(c->gC, g64, sizeof g64); memcpy(c->dC, d64, sizeof d64); }
    else            { c->Lg = 5; c->Ld = 5; memcpy(c->gC, g128, sizeof g128); memcpy(c->dC, d128, sizeof d128); }
    c->F = c->gC[0] * 16;
    c->g_bn_off[0] = 0; c->bn_total = c->F;
    for (int l = 1; l <= c->Lg; ++l) { c->g_bn_off[l] = c->bn_total; c->bn_total += c->gC[l]; }
    // The arenas, in parameters() order, as the records of what is derived from each tensor (struct Derived): a tensor of n
    // elements, followed, n2 > 0, by the one it is paired with
    c->g_total = c->d_total = 0;
    auto rec = [c](int w, int kind, int layer, int64_t n, int64_t n2, int A = 0, int Bc = 0) {
        auto& off = w == 0 ? c->g_off : c->d_off;
        auto& num = w == 0 ? c->g_num : c->d_num;
        int64_t& tot = w == 0 ? c->g_total : c->d_total;
        Derived r; memset(&r, 0, sizeof r);
        r.kind = kind; r.layer = layer; r.A = A; r.Bc = Bc; r.off = tot; r.n = n; r.n2 = n2;
        if (n2) r.off2 = tot + n;
        if (kind == DV_BN) r.bn_off = c->g_bn_off[layer];
        for (int64_t k : {n, n2}) if (k) { off.push_back(tot); num.push_back(k); tot += k; }
        c->rec[w].push_back(r);
    };
    rec(0, DV_FC, 0, (int64_t)c->F * c->latent, c->F, c->latent, c->gC[0]);
    for (int l = 0; l <= c->Lg; ++l) {
        const int C = l == 0 ? c->F : c->gC[l];
        if (l > 0) rec(0, DV_CONV, l, (int64_t)c->gC[l - 1] * C * 16, 0, c->gC[l - 1], C);
        rec(0, DV_BN, l, C, C, C, l == 0 ? c->gC[0] : 0);
    }
    rec(0, DV_TAPS, c->Lg, (int64_t)c->gC[c->Lg] * 9, 1, c->gC[c->Lg], 9);
    rec(1, DV_TAPS, 1, (int64_t)c->dC[1] * 16, c->dC[1], c->dC[1], 16);
    for (int l = 2; l <= c->Ld; ++l) {
        rec(1, DV_CONV, l, (int64_t)c->dC[l] * c->dC[l - 1] * 16, 0, c->dC[l], c->dC[l - 1]);
        rec(1, DV_FLAT, l, c->dC[l], 0);
    }
    rec(1, DV_T16, c->Ld + 1, (int64_t)c->dC[c->Ld] * 16, 0, c->dC[c->Ld]);
    rec(1, DV_FLAT, c->Ld + 1, 1, 0);
}

// A D(real) forward that siggan_g_grads started ahead of time on lane c (siggan_stage_real) and that no D step will
// consume still reads the staged batch, the D weight packs and slab_k2 and writes activation rows [0,B): whoever
// abandons it marks it orphaned, and the next call that enqueues anything first makes its stream wait for that lane.
void siggan::drop_dreal(siggan_ctx* c) {
    if (c->cs.dreal_B) { c->cs.dreal_orphan = true; c->cs.dreal_B = 0; }
}
int siggan::settle(siggan_ctx* c, hipStream_t s) {
    if (c->cs.dreal_orphan) {
        HIPCHK(hipStreamWaitEvent(s, c->ev_dreal, 0));
        c->cs.dreal_orphan = false;
    }
    return SIGGAN_OK;
}
// (the reasons and why their order matters: enum Inval, ctx.h)
void siggan::invalidate(siggan_ctx* c, Inval why) {
    Carried& cs = c->cs;
    switch (why) {
    case INV_INIT:    cs = Carried{};                                                  [[fallthrough]];
    case INV_REBIND:  cs.pending = 0; cs.staged_B = 0;                                 [[fallthrough]];
    case INV_WEIGHTS: c->g_dirty = c->d_dirty = true; c->adam_t_known[0] = c->adam_t_known[1] = false; cs.early_ar = false; [[fallthrough]];
    case INV_ROWS:    cs.conv1_rode = 0;                                               [[fallthrough]];
    case INV_STREAM:  drop_dreal(c); break;
    case INV_COMM:    cs.early_ar = false; break;
    }
}

// The fp32 value of a byte of a generated image as the reference's realism filter feeds it to the Discriminator
// (app_vanilla_gan_signatures.py:1364-1372, torch.from_numpy(b).float() / 127.5 - 1.0 on the CPU): a correctly rounded fp32
// division, then a separate fp32 subtraction -- two roundings.  Formed here on the host (the file is built without contraction),
// so no device division or reciprocal has a say in it.
static void dequant_table(float* lut) {
    for (int b = 0; b < 256; ++b) {
        volatile float q = (float)b / 127.5f;
        lut[b] = q - 1.0f;
    }
}
extern "C" int siggan_dequant_table(float* table_host) {
    if (!table_host) return FAIL(SIGGAN_E_INVALID, "null table");
    dequant_table(table_host);
    return SIGGAN_OK;
}

extern "C" int siggan_create(const siggan_config* cfg, siggan_ctx** out) {
    if (!cfg || !out) return FAIL(SIGGAN_E_INVALID, "null argument");
    if (cfg->image_size != 64 && cfg->image_size != 128)
        return FAIL(SIGGAN_E_INVALID, "output_size must be 64 or 128, got %d", cfg->image_size);
    if (cfg->image_channels != 1) return FAIL(SIGGAN_E_INVALID, "only image_channels == 1 is built, got %d", cfg->image_channels);
    if (cfg->latent_dim < 1 || cfg->latent_dim > 4096) return FAIL(SIGGAN_E_INVALID, "latent_dim out of range: %d", cfg->latent_dim);
    if (cfg->max_batch < 1 || cfg->max_batch > 4096) return FAIL(SIGGAN_E_INVALID, "max_batch out of range: %d", cfg->max_batch);
    if (!(cfg->dropout >= 0.f && cfg->dropout < 1.f)) return FAIL(SIGGAN_E_INVALID, "dropout must be in [0,1)");
    if (cfg->dtype != SIGGAN_DTYPE_F32 && cfg->dtype != SIGGAN_DTYPE_BF16 && cfg->dtype != SIGGAN_DTYPE_F16)
        return FAIL(SIGGAN_E_INVALID, "dtype must be SIGGAN_DTYPE_F32, _BF16 or _F16, got %d", cfg->dtype);
    if (!(cfg->f16_grad_scale >= 0.f) || cfg->f16_grad_scale > 65536.f)
        return FAIL(SIGGAN_E_INVALID, "f16_grad_scale must be in [0, 65536] (0 = default)");
    if (!(cfg->g_leaky_slope >= 0.f) || !isfinite(cfg->g_leaky_slope))
        return FAIL(SIGGAN_E_INVALID, "g_leaky_slope must be finite and >= 0 (0 = ReLU), got %g", (double)cfg->g_leaky_slope);
    DevGuard dg(cfg->device);
    HIPCHK(dg.err);
    siggan_ctx* c = new (std::nothrow) siggan_ctx();
    if (!c) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    c->cfg = *cfg; c->S = cfg->image_size; c->latent = cfg->latent_dim; c->Bm = cfg->max_batch;
    c->dt = cfg->dtype; c->es = dt_size(c->dt);
    c->fc_fused = cfg->max_batch <= 256 && (cfg->latent_dim & 3) == 0;
    c->variant = SIGGAN_STEP_TRAINER;
    c->sn = cfg->spectral_norm != 0;
    // fp16 stores activation gradients of order 1e-7..1e-3: a power-of-two scale (exact to apply and to remove) lifts
    // them clear of the fp16 subnormals; bf16 has fp32's exponent range and needs none
    c->gscale = c->dt == DT_F16 ? (cfg->f16_grad_scale > 0.f ? cfg->f16_grad_scale : 1024.f) : 1.0f;
    c->bound = false;
    invalidate(c, INV_INIT);
    build_layout(c);

    // ---- workspace carve (two passes: size, then assign) ----------------------------------
    const int64_t Bm = c->Bm, Bd = 2 * Bm;
    size_t off = 0;
    char* base = nullptr;
    auto carve = [&](float** p, int64_t nfloats) {
        if (base) *p = (float*)(base + off);
        off += ((size_t)nfloats * sizeof(float) + 255) & ~(size_t)255;
    };
    auto carve_t = [&](char** p, int64_t nelem) {          // a tensor of the context's element type
        if (base) *p = base + off;
        off += ((size_t)nelem * c->es + 255) & ~(size_t)255;
    };
    c->slab_floats = (int64_t)16 << 20;
    c->slab_k_floats = (int64_t)16 << 20;
    for (int pass = 0; pass < 2; ++pass) {
        off = 0;
        carve(&c->z, Bm * c->latent);
        carve_t(&c->fc_y, Bm * c->F);
        for (int l = 0; l <= c->Lg; ++l) {
            const int64_t H = 4 << l, n = Bm * H * H * c->gC[l];
            if (l == 0) c->g_y[0] = c->fc_y; else carve_t(&c->g_y[l], n);
            carve_t(&c->g_a[l], n);
            if (c->dt != DT_F32) carve_t(&c->g_ae[l], n); else if (pass == 1) c->g_ae[l] = c->g_a[l];
            carve_t(&c->g_da[l], n);
            carve(&c->g_bn[l], 6 * (int64_t)(l == 0 ? c->F : c->gC[l]));
            carve(&c->g_bne[l], 4 * (int64_t)(l == 0 ? c->F : c->gC[l]));   // eval-mode [scale|shift|mean|rstd]
        }
        if (pass == 1) c->g_y[0] = c->fc_y;
        carve(&c->img, Bm * c->S * c->S);
        carve(&c->dpre, Bm * c->S * c->S);
        for (int l = 1; l <= c->Ld; ++l) {
            const int64_t H = c->S >> l, n = Bd * H * H * c->dC[l];
            carve_t(&c->d_a[l], n);
            carve_t(&c->d_dv[l], n);
            carve(&c->d_noise[l], Bd * c->dC[l]);
        }
        carve(&c->logits, Bd); carve(&c->probs, Bd); carve(&c->dlogit, Bd);
        carve(&c->lparts, (int64_t)Bd * 16);
        for (int l = 1; l <= c->Lg; ++l) {
            carve_t(&c->g_up[l], (int64_t)c->gC[l - 1] * c->gC[l] * 16);
            carve_t(&c->g_dn[l], (int64_t)c->gC[l - 1] * c->gC[l] * 16);
        }
        for (int l = 2; l <= c->Ld; ++l) {
            carve_t(&c->d_dn[l], (int64_t)c->dC[l - 1] * c->dC[l] * 16);
            carve_t(&c->d_up[l], (int64_t)c->dC[l - 1] * c->dC[l] * 16);
        }
        carve(&c->wcp, (int64_t)c->dC[c->Ld] * 16);
        carve(&c->slab, c->slab_floats);
        carve(&c->slab_k, c->slab_k_floats);
        if (c->dt != DT_F32) carve(&c->slab_b, c->slab_floats); else if (pass == 1) c->slab_b = c->slab;
        carve(&c->slab_k2, c->slab_k_floats);
        if (c->dt != DT_F32) carve(&c->slab_k3, c->slab_k_floats); else if (pass == 1) c->slab_k3 = c->slab_k2;
        carve(&c->partial, PARTIAL_FLOATS);
        carve(&c->partial_b, PARTIAL_FLOATS);
        carve(&c->partial_c, PARTIAL_FLOATS);
        carve(&c->z_g, Bm * c->latent);
        carve(&c->img_g, Bm * c->S * c->S);
        carve(&c->real_stage, Bm * c->S * c->S);
        { int64_t sumC = 0; for (int l = 1; l <= c->Ld; ++l) sumC += c->dC[l]; carve(&c->mask_stage, 3 * Bm * sumC); }
        if (c->sn) {
            int64_t ut = 1, vt = (int64_t)c->dC[c->Ld] * 16;
            for (int l = 1; l <= c->Ld; ++l) { ut += c->dC[l]; vt += (int64_t)c->dC[l - 1] * 16; }
            carve(&c->sn_tbuf, vt); carve(&c->sn_wbuf, ut);
            carve(&c->sn_sig, 3 * 2 * SnTable::MAXS);
            carve(&c->sn_us, 3 * ut); carve(&c->sn_vs, 3 * vt);
            carve(&c->sn_dots, 2 * SnTable::MAXS * 64);
            carve(&c->sn_g[0], c->d_total); carve(&c->sn_g[1], c->d_total);
            carve(&c->d_w1s, (int64_t)c->dC[1] * 16);
        }
        carve(&c->metrics, SIGGAN_M_COUNT);
        carve_t(&c->op_pack, (int64_t)512 * 512 * 16);
        carve(&c->zeros, 64);
        carve(&c->wfc_t, (int64_t)c->F * c->latent);
        carve(&c->wfin_t, (int64_t)9 * c->gC[c->Lg]);
        carve(&c->d_w1t, (int64_t)16 * c->dC[1]);
        carve(&c->ride_ctr, 64);
        carve(&c->deq_lut, 256);
        carve(&c->ones, 64);
        { int64_t sumC = 0; for (int l = 1; l < c->Lg; ++l) sumC += c->gC[l]; carve(&c->lg_tab, Bm * sumC); }
        float* devp = nullptr;
        carve(&devp, 64);
        if (pass == 1) c->dev = (DevState*)devp;
        if (pass == 0) {
            c->ws_bytes = off;
            hipError_t e = hipMalloc((void**)&base, off);
            if (e != hipSuccess) { delete c; return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", off, hipGetErrorString(e)); }
            c->ws = base;
        }
    }
    for (int w = 0; w < 2; ++w) {                      // where each record's derived tensors live; can the update be k_adam_pack
        bool ok = w == 0 || !c->sn;
        for (Derived& r : c->rec[w]) {
            const int l = r.layer;
            switch (r.kind) {
            case DV_FC:   r.dst = c->fc_fused ? nullptr : c->wfc_t; ok = ok && c->fc_fused; break;
            case DV_CONV: r.dst = (float*)(w ? c->d_dn : c->g_dn)[l]; r.dst2 = (float*)(w ? c->d_up : c->g_up)[l];
                          ok = ok && r.A % 16 == 0 && r.Bc % 16 == 0; break;
            case DV_BN:   r.dst = c->g_bne[l]; break;
            case DV_TAPS: r.dst = w ? c->d_w1t : c->wfin_t; r.dst2 = w && c->sn ? c->d_w1s : nullptr;
                          ok = ok && r.n <= 1024 && r.n2 <= 256; break;
            case DV_T16:  r.dst = c->wcp; break;
            }
        }
        c->packable[w] = ok;
    }
    HIPCHK(hipMemset(c->ws, 0, c->ws_bytes));
    DevState h; memset(&h, 0, sizeof h);
    h.seed = cfg->seed; h.rng_ctr = 0; h.grad_mul = 1.f;
    HIPCHK(hipMemcpy(c->dev, &h, sizeof h, hipMemcpyHostToDevice));
    { float lut[256]; dequant_table(lut); HIPCHK(hipMemcpy(c->deq_lut, lut, sizeof lut, hipMemcpyHostToDevice)); }
    { float one[64]; for (float& v : one) v = 1.0f; HIPCHK(hipMemcpy(c->ones, one, sizeof one, hipMemcpyHostToDevice)); }
    c->mode = SIGGAN_MODE_OVERLAP;   // hipGraph replay measured slower than eager launches on ROCm 7
    c->evi = 0;
    HIPCHK(hipStreamCreateWithFlags(&c->s_m, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->s_a, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->s_b, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->s_c, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->s_n, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_gfwd, EV_FLAGS));
    HIPCHK(hipEventCreateWithFlags(&c->ev_dreal, EV_FLAGS));
    HIPCHK(hipEventCreateWithFlags(&c->ev_ar, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_sys[i], hipEventDisableTiming));
    c->lane_err = hipSuccess;
    c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1; c->comm_err = 0;
    HIPCHK(hipHostMalloc((void**)&c->ride_late, sizeof(unsigned), hipHostMallocCoherent | hipHostMallocMapped));
    *c->ride_late = 0u;
    HIPCHK(hipHostGetDevicePointer((void**)&c->ride_late_dev, c->ride_late, 0));
    for (int i = 0; i < siggan_ctx::NEV; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev[i], EV_FLAGS));
    for (int i = 0; i < siggan_ctx::NEV; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_fenced[i], hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_bridge[i], hipEventDisableTiming));
    *out = c;
    return SIGGAN_OK;
}

extern "C" int siggan_destroy(siggan_ctx* c) {
    if (!c) return SIGGAN_OK;
    DevGuard dg(c->cfg.device);
    (void)hipDeviceSynchronize();
    if (c->comm) { (void)rccl()->CommDestroy(c->comm); c->comm = nullptr; }
    for (auto& e : c->graphs) (void)hipGraphExecDestroy(e.exec);
    for (int i = 0; i < siggan_ctx::NEV; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < siggan_ctx::NEV; ++i) if (c->ev_fenced[i]) (void)hipEventDestroy(c->ev_fenced[i]);
    for (int i = 0; i < 2; ++i) if (c->ev_bridge[i]) (void)hipEventDestroy(c->ev_bridge[i]);
    if (c->s_m) (void)hipStreamDestroy(c->s_m);
    if (c->s_a) (void)hipStreamDestroy(c->s_a);
    if (c->s_b) (void)hipStreamDestroy(c->s_b);
    if (c->s_c) (void)hipStreamDestroy(c->s_c);
    if (c->s_n) (void)hipStreamDestroy(c->s_n);
    if (c->ev_ar) (void)hipEventDestroy(c->ev_ar);
    for (int i = 0; i < 2; ++i) if (c->ev_sys[i]) (void)hipEventDestroy(c->ev_sys[i]);
    if (c->ev_gfwd) (void)hipEventDestroy(c->ev_gfwd);
    if (c->ev_dreal) (void)hipEventDestroy(c->ev_dreal);
    if (c->ws) (void)hipFree(c->ws);
    if (c->ride_late) (void)hipHostFree(c->ride_late);
    delete c;
    return SIGGAN_OK;
}

extern "C" int64_t siggan_param_count(const siggan_ctx* c, int which) { return !c ? -1 : (which == 0 ? c->g_total : c->d_total); }
extern "C" int32_t siggan_param_tensors(const siggan_ctx* c, int which) {
    return !c ? -1 : (int32_t)(which == 0 ? c->g_off.size() : c->d_off.size());
}
extern "C" int siggan_param_span(const siggan_ctx* c, int which, int32_t idx, int64_t* offset, int64_t* numel) {
    if (!c || !offset || !numel) return FAIL(SIGGAN_E_INVALID, "null argument");
    const auto& o = which == 0 ? c->g_off : c->d_off;
    const auto& n = which == 0 ? c->g_num : c->d_num;
    if (idx < 0 || idx >= (int32_t)o.size()) return FAIL(SIGGAN_E_INVALID, "tensor index %d out of range", idx);
    *offset = o[idx]; *numel = n[idx];
    return SIGGAN_OK;
}
extern "C" int64_t siggan_bn_count(const siggan_ctx* c) { return c ? c->bn_total : -1; }
extern "C" int64_t siggan_sn_count(const siggan_ctx* c, int which) {
    if (!c) return -1;
    int64_t ut = 1, vt = (int64_t)c->dC[c->Ld] * 16;
    for (int l = 1; l <= c->Ld; ++l) { ut += c->dC[l]; vt += (int64_t)c->dC[l - 1] * 16; }
    return which == 0 ? ut : vt;
}
extern "C" int32_t siggan_bn_layers(const siggan_ctx* c) { return c ? c->Lg + 1 : -1; }
extern "C" int64_t siggan_workspace_bytes(const siggan_ctx* c) { return c ? (int64_t)c->ws_bytes : -1; }

extern "C" int siggan_bind(siggan_ctx* c, const siggan_storage* st) {
    if (!c || !st) return FAIL(SIGGAN_E_INVALID, "null argument");
    const void* need[] = {st->g_params, st->g_bn_running_mean, st->g_bn_running_var, st->d_params};
    for (const void* p : need)
        if (!p) return FAIL(SIGGAN_E_INVALID, "siggan_bind: parameters and BatchNorm buffers are required");
    const void* all[] = {st->g_params, st->g_grads, st->g_exp_avg, st->g_exp_avg_sq, st->d_params, st->d_grads,
                         st->d_exp_avg, st->d_exp_avg_sq};
    for (const void* p : all)
        if (((uintptr_t)p & 15) != 0) return FAIL(SIGGAN_E_INVALID, "siggan_bind: arenas must be 16-byte aligned");
    c->st = *st;
    if (c->sn) {
        if (!st->d_sn_u || !st->d_sn_v) return FAIL(SIGGAN_E_INVALID, "siggan_bind: a spectral-norm context needs d_sn_u / d_sn_v");
        SnTable& t = c->snt; memset(&t, 0, sizeof t);
        t.n = c->Ld + 1;
        int uo = 0, vo = 0;
        t.pre_k[0] = t.pre_r[0] = 0;
        for (int i = 0; i < t.n; ++i) {
            SnLayer& L = t.layer[i];
            const bool cls = i == c->Ld;
            const int pi = cls ? di_cls_w(c) : di_w(i + 1);
            L.W = st->d_params + c->d_off[pi]; L.w_off = c->d_off[pi];
            L.rows = cls ? 1 : c->dC[i + 1]; L.K = cls ? c->dC[c->Ld] * 16 : c->dC[i] * 16;
            L.u_off = uo; L.v_off = vo; uo += L.rows; vo += L.K;
            t.pre_k[i + 1] = t.pre_k[i] + (L.K + 255) / 256;
            t.pre_r[i + 1] = t.pre_r[i] + (L.rows + 3) / 4;
        }
        t.u = st->d_sn_u; t.v = st->d_sn_v; t.tbuf = c->sn_tbuf; t.wbuf = c->sn_wbuf; t.sig = c->sn_sig;
        t.u_saved = c->sn_us; t.v_saved = c->sn_vs; t.dots = c->sn_dots; t.u_total = uo; t.v_total = vo;
    }
    c->bound = true;
    invalidate(c, INV_REBIND);
    return SIGGAN_OK;
}
extern "C" int siggan_params_changed(siggan_ctx* c) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    invalidate(c, INV_WEIGHTS);        // (optimizer.load_state_dict writes the step tensors too)
    return SIGGAN_OK;
}
extern "C" int siggan_seed(siggan_ctx* c, uint64_t seed, uint64_t offset) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    unsigned long long v[2] = {seed, offset};
    HIPCHK(hipMemcpy(c->dev, v, sizeof v, hipMemcpyHostToDevice));   // seed, rng_ctr are the first two fields
    invalidate(c, INV_STREAM);
    return SIGGAN_OK;
}

extern "C" int siggan_rng_state(siggan_ctx* c, uint64_t* seed, uint64_t* offset) {
    ENTER(c);
    if (!seed || !offset) return FAIL(SIGGAN_E_INVALID, "null argument");
    HIPCHK(hipDeviceSynchronize());
    unsigned long long v[2];
    HIPCHK(hipMemcpy(v, c->dev, sizeof v, hipMemcpyDeviceToHost));
    *seed = v[0]; *offset = v[1];
    return SIGGAN_OK;
}

// A training-mode Generator forward of ONE sample: the fc block's BatchNorm1d has a single value per channel, which torch
// refuses (torch/nn/functional.py _verify_batch_size, reached from generator_vanilla_gan.py:112) -- same refusal, same text
// (the binding raises ValueError for SIGGAN_E_INVALID, as torch does).  Eval mode and the Discriminator take one sample.
int siggan::check_bn_batch(const siggan_ctx* c, int batch) {
    if (batch == 1)
        return FAIL(SIGGAN_E_INVALID, "Expected more than 1 value per channel when training, got input size torch.Size([1, %d])", c->F);
    return SIGGAN_OK;
}
int siggan::check_call(siggan_ctx* c, int batch, bool need_bound) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    if (need_bound && !c->bound) return FAIL(SIGGAN_E_STATE, "siggan_bind has not been called");
    if (batch < 1 || batch > c->Bm) return FAIL(SIGGAN_E_INVALID, "batch %d outside [1, max_batch=%d]", batch, c->Bm);
    return SIGGAN_OK;
}

int siggan::lane_check(siggan_ctx* c) {
    if (c->comm_err)      // sticky: the communicator is unusable and the replicas have diverged; cleared by siggan_comm_destroy
        return FAIL(SIGGAN_E_HIP, "ncclAllReduce of the gradient bucket failed (the optimiser update was skipped): %s",
                    rccl()->GetErrorString(c->comm_err));
    // sticky: set by the device (k_adam_pack) when its owner of the block-1 ranges stopped waiting for the riders -- a late
    // rider then ran the G step's first Discriminator block on weights updated twice.  Seen once that launch has run.
    if (c->ride_late && __atomic_load_n(c->ride_late, __ATOMIC_ACQUIRE))
        return FAIL(SIGGAN_E_STATE, "riders did not report: the optimiser update's owner of the first Discriminator block stopped "
                                    "waiting for them (a G step's first block may have used twice-updated weights)");
    if (c->refused) return FAIL(SIGGAN_E_STATE, "%s", c->refused);
    if (c->lane_err == hipSuccess) return SIGGAN_OK;
    const hipError_t e = c->lane_err; c->lane_err = hipSuccess;
    return FAIL(SIGGAN_E_HIP, "an event record / stream wait / prepare table of the step failed: %s", hipGetErrorString(e));
}

extern "C" int siggan_set_step_variant(siggan_ctx* c, int32_t variant) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    if (variant != SIGGAN_STEP_TRAINER && variant != SIGGAN_STEP_ABLATION) return FAIL(SIGGAN_E_INVALID, "unknown step variant %d", variant);
    if (c->cs.g_fwd_pending || c->cs.pending) return FAIL(SIGGAN_E_STATE, "a step is in flight");
    c->variant = variant;
    return SIGGAN_OK;
}

extern "C" int siggan_set_mode(siggan_ctx* c, int32_t mode) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    c->mode = mode;
    return SIGGAN_OK;
}

extern "C" int siggan_device_info(int32_t device, int32_t* compute_units, int32_t* clock_khz, int64_t* hbm_bytes) {
    if (!compute_units || !clock_khz || !hbm_bytes) return FAIL(SIGGAN_E_INVALID, "null argument");
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, device));
    *compute_units = p.multiProcessorCount; *clock_khz = p.clockRate; *hbm_bytes = (int64_t)p.totalGlobalMem;
    return SIGGAN_OK;
}
