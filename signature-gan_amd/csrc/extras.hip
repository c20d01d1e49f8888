// extras.hip -- the C ABI's entry points beside the model: single operators, the data-parallel communicator, the launch
// profiler, the debug tensors, and the input pipeline's and image statistics' shims.  Host code only.
#include "ctx.h"

// ---- operator-level entry points ----------------------------------------------------------
static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" int siggan_op_conv4x4s2(siggan_ctx* c, int32_t form, const void* in_dev, const float* w_dev, void* out_dev,
                                   int32_t batch, int32_t h_in, int32_t c_in, int32_t c_out, void* stream) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    if (!in_dev || !w_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (form != 0 && form != 1) return FAIL(SIGGAN_E_INVALID, "form must be 0 (down) or 1 (up)");
    if (!pow2(h_in) || !pow2(c_in) || !pow2(c_out) || c_in < 32 || c_out < 32 || c_in > 512 || c_out > 512 || batch < 1)
        return FAIL(SIGGAN_E_INVALID, "shape not in the model family (pow2 dims, 32 <= C <= 512)");
    if (form == 0 && h_in < 2) return FAIL(SIGGAN_E_INVALID, "down form needs h_in >= 2");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    hipStream_t s = (hipStream_t)stream;
    GConvArgs a = gconv_args(c, form, batch, h_in, c_in, c_out);
    a.in = in_dev; a.wp = c->op_pack; a.out = out_dev; a.epi = EPI_RAW;
    PrepTable t; t.njobs = 0; t.overflow = 0;
    PrepJob j; memset(&j, 0, sizeof j);
    j.src = w_dev; j.dst = (float*)c->op_pack; j.dt = c->dt;
    if (form == 0) { j.type = PREP_PACK_DOWN; j.O = c_out; j.I = c_in; }
    else           { j.type = PREP_PACK_UP; j.I = c_in; j.O = c_out; }
    prep_add(t, j);
    if (!launch_prepare(t, BN_EPS, s)) return FAIL(SIGGAN_E_STATE, "prepare table overflow");
    launch_gconv(a, s);
    LAUNCHCHK();
    return SIGGAN_OK;
}

extern "C" int siggan_op_conv4x4s2_wgrad(siggan_ctx* c, const void* small_dev, const void* large_dev, float* dw_dev,
                                         int32_t batch, int32_t h_small, int32_t c_small, int32_t c_large, void* stream) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    if (!small_dev || !large_dev || !dw_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (!pow2(h_small) || !pow2(c_small) || !pow2(c_large) || c_small < 32 || c_large < 32 || c_small > 512 || c_large > 512 ||
        batch < 1)
        return FAIL(SIGGAN_E_INVALID, "shape not in the model family (pow2 dims, 32 <= C <= 512)");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    hipStream_t s = (hipStream_t)stream;
    const WgradCall g = wgrad_args(c, small_dev, large_dev, dw_dev, c->slab, batch, h_small, c_small, c_large);
    launch_wgrad(g.w, g.max_splits, s);
    LAUNCHCHK();
    return SIGGAN_OK;
}

extern "C" int siggan_op_adam(siggan_ctx* c, float* p, float* g, float* m, float* v, int64_t n, int32_t step,
                              const siggan_hyper* hp, void* stream) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    int rc = check_hyper(hp);
    if (rc) return rc;
    if (!p || !g || !m || !v || n < 1 || step < 1) return FAIL(SIGGAN_E_INVALID, "bad argument");
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) != 0) return FAIL(SIGGAN_E_INVALID, "arenas must be 16-byte aligned");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    hipStream_t s = (hipStream_t)stream;
    float* steps = c->partial + ((2 << 20) - 64);          // scratch slot: step count before the increment
    const float prev = (float)(step - 1);
    HIPCHK(hipMemcpyAsync(steps, &prev, sizeof prev, hipMemcpyHostToDevice, s));
    const bool clip = hp->clip_max_norm > 0.f;
    const float gs = hp->grad_scale > 0.f ? hp->grad_scale : 1.0f;
    if (clip) launch_grad_sumsq(g, n, c->partial, s);
    launch_adam_prepare(c->dev, steps, 1, hp->lr, hp->beta1, hp->beta2, gs, hp->clip_max_norm, nullptr, s, 0, nullptr,
                        clip ? c->partial : nullptr);
    launch_adam(p, g, m, v, n, c->dev, hp->beta1, hp->beta2, hp->eps, (clip || gs != 1.0f) ? 1 : 0, s);
    LAUNCHCHK();
    return SIGGAN_OK;
}

extern "C" int siggan_op_anchor(siggan_ctx* c, float* g, const float* p, const float* p0, int64_t n, float weight, void* stream) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    if (!g || !p || !p0 || n < 1) return FAIL(SIGGAN_E_INVALID, "bad argument");
    if (!isfinite(weight) || weight < 0.f) return FAIL(SIGGAN_E_INVALID, "weight must be finite and >= 0, got %g", (double)weight);
    if ((((uintptr_t)g | (uintptr_t)p | (uintptr_t)p0) & 3) != 0) return FAIL(SIGGAN_E_INVALID, "tensors must be 4-byte aligned");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    launch_anchor(g, p, p0, n, weight, (hipStream_t)stream);
    LAUNCHCHK();
    return SIGGAN_OK;
}

// ---- data-parallel communicator (the Rccl table and why it is resolved at run time: ctx.h) --
Rccl* siggan::rccl() {
    static Rccl r;
    if (r.h || r.err) return &r;
    const char* names[] = {"librccl.so.1", "librccl.so"};
    for (const char* n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);      // the copy torch loaded
    for (const char* n : names) if (!r.h) r.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!r.h) { r.err = "librccl.so was not found (load it, or import torch, before siggan_comm_*)"; return &r; }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.h, "ncclCommDestroy");
    r.AllReduce = (decltype(r.AllReduce))dlsym(r.h, "ncclAllReduce");
    r.Broadcast = (decltype(r.Broadcast))dlsym(r.h, "ncclBroadcast");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(r.h, "ncclGetErrorString");
    if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllReduce || !r.Broadcast || !r.GetErrorString)
        r.err = "librccl.so lacks one of ncclGetUniqueId / CommInitRank / CommDestroy / AllReduce / Broadcast / GetErrorString";
    return &r;
}
#define NCCLCHK(x)                                                                                  \
    do {                                                                                            \
        int e_ = (x);                                                                               \
        if (e_ != NCCL_SUCCESS) return FAIL(SIGGAN_E_HIP, "%s -> %s (%s:%d)", #x, rccl()->GetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
extern "C" int siggan_comm_unique_id(void* id_out) {
    if (!id_out) return FAIL(SIGGAN_E_INVALID, "null argument");
    Rccl* r = rccl();
    if (r->err) return FAIL(SIGGAN_E_STATE, "%s", r->err);
    ncclUniqueId_t id;
    NCCLCHK(r->GetUniqueId(&id));
    memcpy(id_out, &id, sizeof id);
    return SIGGAN_OK;
}
extern "C" int siggan_comm_init(siggan_ctx* c, int32_t rank, int32_t world, const void* id) {
    ENTER(c);
    if (!id || world < 1 || rank < 0 || rank >= world) return FAIL(SIGGAN_E_INVALID, "bad rank / world / id");
    if (c->comm) return FAIL(SIGGAN_E_STATE, "a communicator is already initialised");
    Rccl* r = rccl();
    if (r->err) return FAIL(SIGGAN_E_STATE, "%s", r->err);
    ncclUniqueId_t uid;
    memcpy(&uid, id, sizeof uid);
    NCCLCHK(r->CommInitRank(&c->comm, world, uid, rank));
    c->comm_rank = rank; c->comm_world = world;
    return SIGGAN_OK;
}
extern "C" int siggan_comm_destroy(siggan_ctx* c) {
    ENTER(c);
    if (!c->comm) return SIGGAN_OK;
    HIPCHK(hipDeviceSynchronize());
    NCCLCHK(rccl()->CommDestroy(c->comm));
    c->comm = nullptr; c->comm_rank = 0; c->comm_world = 1; c->comm_err = 0;
    invalidate(c, INV_COMM);
    return SIGGAN_OK;
}
extern "C" int32_t siggan_comm_world(const siggan_ctx* c) { return c ? c->comm_world : -1; }
extern "C" int siggan_comm_broadcast(siggan_ctx* c, void* buf_dev, int64_t bytes, int32_t root, void* stream) {
    ENTER(c);
    if (!buf_dev || bytes < 1 || root < 0 || root >= c->comm_world) return FAIL(SIGGAN_E_INVALID, "bad argument");
    if (!c->comm) return SIGGAN_OK;                      // a single replica already holds the root's bytes
    NCCLCHK(rccl()->Broadcast(buf_dev, buf_dev, (size_t)bytes, NCCL_CHAR, root, c->comm, (hipStream_t)stream));
    return SIGGAN_OK;
}

static Prof g_prof_store;
extern "C" int siggan_prof_enable(siggan_ctx* c, int32_t on) {
    if (!c) return FAIL(SIGGAN_E_INVALID, "null context");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    HIPCHK(hipDeviceSynchronize());
    g_prof_store.clear();
    g_prof = on ? &g_prof_store : nullptr;
    return SIGGAN_OK;
}
extern "C" int32_t siggan_prof_slots(void) { return Prof::NID - 1; }
extern "C" int siggan_prof_read(siggan_ctx* c, int32_t idx, char* name, int32_t name_cap, int64_t* launches, double* ms,
                                double* flops, double* bytes) {
    if (!c || !name || !launches || !ms || !flops || !bytes || idx < 0 || idx >= Prof::NID - 1) return FAIL(SIGGAN_E_INVALID, "bad argument");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    HIPCHK(hipDeviceSynchronize());
    snprintf(name, name_cap, "%s", Prof::name(idx));
    *launches = 0; *ms = 0.0; *flops = 0.0; *bytes = 0.0;
    for (auto& r : g_prof_store.recs) {
        if (r.id != idx) continue;
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, r.e0, r.e1));
        *launches += 1; *ms += t; *flops += r.flops; *bytes += r.bytes;
    }
    return SIGGAN_OK;
}

extern "C" int siggan_prof_launch(siggan_ctx* c, int64_t idx, int32_t* fields, int32_t n, int64_t* count) {
    if (!c || !count || (n > 0 && !fields)) return FAIL(SIGGAN_E_INVALID, "bad argument");
    *count = (int64_t)g_prof_store.recs.size();
    if (n <= 0) return SIGGAN_OK;
    if (idx < 0 || idx >= *count) return FAIL(SIGGAN_E_INVALID, "launch %lld of %lld", (long long)idx, (long long)*count);
    const Prof::Rec& r = g_prof_store.recs[(size_t)idx];
    const int32_t v[9] = {r.id, r.form, r.epi_req, r.epi, r.M, r.Ci, r.Co, r.slabs, r.kq};
    for (int i = 0; i < n && i < 9; ++i) fields[i] = v[i];
    return SIGGAN_OK;
}

extern "C" int siggan_debug_tensor(siggan_ctx* c, const char* name, int32_t idx, float* out_dev, int64_t n, void* stream) {
    if (!c || !name || !out_dev || n < 1) return FAIL(SIGGAN_E_INVALID, "bad argument");
    const void* src = nullptr; int64_t capv = 0;
    const void** ptr = &src; int64_t* cap = &capv;
    bool typed = true;                          // element type dt (converted to fp32 on the way out) vs. plain fp32
    const int64_t Bm = c->Bm, Bd = 2 * Bm, SS = (int64_t)c->S * c->S;
    auto gsz = [&](int l) { const int64_t H = 4 << l; return Bm * H * H * c->gC[l]; };
    auto dsz = [&](int l) { const int64_t H = c->S >> l; return Bd * H * H * c->dC[l]; };
    const bool gl = idx >= 0 && idx <= c->Lg, dl = idx >= 1 && idx <= c->Ld;
    if (!strcmp(name, "g_y") && gl) { *ptr = c->g_y[idx]; *cap = gsz(idx); }
    else if (!strcmp(name, "g_a") && gl) { *ptr = c->g_a[idx]; *cap = gsz(idx); }
    else if (!strcmp(name, "g_da") && gl) { *ptr = c->g_da[idx]; *cap = gsz(idx); }
    else if (!strcmp(name, "d_a") && dl) { *ptr = c->d_a[idx]; *cap = dsz(idx); }
    else if (!strcmp(name, "d_dv") && dl) { *ptr = c->d_dv[idx]; *cap = dsz(idx); }
    else if (!strcmp(name, "d_a_g") && dl) {     // the Discriminator activations of the last G step (they may start at row B)
        const int64_t H = c->S >> idx, off = (int64_t)c->cs.g_r0 * H * H * c->dC[idx];
        *ptr = c->d_a[idx] + (size_t)off * c->es; *cap = dsz(idx) - off;
    }
    else if (!strcmp(name, "z")) { *ptr = c->z; *cap = Bm * c->latent; typed = false; }
    else if (!strcmp(name, "z_g")) { *ptr = c->z_g; *cap = Bm * c->latent; typed = false; }
    else if (!strcmp(name, "img")) { *ptr = c->img; *cap = Bm * SS; typed = false; }
    else if (!strcmp(name, "dpre")) { *ptr = c->dpre; *cap = Bm * SS; typed = false; }
    else if (!strcmp(name, "logits")) { *ptr = c->logits; *cap = Bd; typed = false; }
    else if (!strcmp(name, "probs")) { *ptr = c->probs; *cap = Bd; typed = false; }
    else if (!strcmp(name, "dlogit")) { *ptr = c->dlogit; *cap = Bd; typed = false; }
    else if (!strcmp(name, "d_noise") && dl) { *ptr = c->d_noise[idx]; *cap = Bd * c->dC[idx]; typed = false; }
    else if (!strcmp(name, "rode") || !strcmp(name, "pre_real") || !strcmp(name, "ride_late")) {
        // host-side scalars (as floats), read once the stream has run (ride_late is written by the device): synchronous
        if (n != 1) return FAIL(SIGGAN_E_INVALID, "debug scalar %s holds 1 float, %lld asked", name, (long long)n);
        DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        const float v = !strcmp(name, "rode") ? (float)c->cs.g_rode : !strcmp(name, "pre_real") ? (float)c->cs.g_pre_real
                                                                                               : (float)__atomic_load_n(c->ride_late, __ATOMIC_ACQUIRE);
        HIPCHK(hipMemcpy(out_dev, &v, sizeof v, hipMemcpyHostToDevice));
        return SIGGAN_OK;
    }
    else return FAIL(SIGGAN_E_INVALID, "unknown debug tensor %s[%d]", name, idx);
    if (n > capv) return FAIL(SIGGAN_E_INVALID, "debug tensor %s[%d] holds %lld floats, %lld asked", name, idx, (long long)capv, (long long)n);
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    if (!strcmp(name, "g_a") && idx == c->Lg && c->cs.ga_last_B) {
        // after a training forward the last block's activation exists only as y + the BatchNorm table: form it now
        const int64_t H = c->S;
        HIPCHK(hipDeviceSynchronize());
        launch_bn_relu(c->dt, c->g_y[idx], c->g_a[idx], (int64_t)c->cs.ga_last_B * H * H, c->gC[idx], c->g_bn[idx], c->cfg.g_leaky_slope,
                       (hipStream_t)stream);
        LAUNCHCHK();
    }
    if (typed && c->dt != DT_F32) { launch_to_f32(c->dt, src, out_dev, n, (hipStream_t)stream); LAUNCHCHK(); }
    else HIPCHK(hipMemcpyAsync(out_dev, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SIGGAN_OK;
}

extern "C" int siggan_augment_batch(int32_t device, const uint8_t* cache_dev, int64_t n_images, const int32_t* index_dev,
                                    const int32_t* params_dev, const int16_t* tables_dev, const float* lut_dev, float* out_dev,
                                    int32_t batch, int32_t size, int32_t augment, int32_t fill, void* stream) {
    if (!cache_dev || !index_dev || !lut_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (augment && (!params_dev || !tables_dev)) return FAIL(SIGGAN_E_INVALID, "augment needs params and tables");
    if (batch < 1 || n_images < 1 || size < 1 || size > 1024) return FAIL(SIGGAN_E_INVALID, "bad batch / cache / image size");
    if (fill < 0 || fill > 255) return FAIL(SIGGAN_E_INVALID, "fill must be a byte value");
    DevGuard dg_(device); HIPCHK(dg_.err);
    launch_augment(cache_dev, n_images, index_dev, params_dev, tables_dev, lut_dev, out_dev, batch, size, augment != 0, fill, (hipStream_t)stream);
    LAUNCHCHK();
    return SIGGAN_OK;
}

extern "C" int siggan_image_stats(int32_t device, const float* x_dev, int32_t batch, int64_t pixels, float threshold,
                                  int32_t* stats_dev, void* stream) {
    if (!x_dev || !stats_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (batch < 1 || pixels < 1) return FAIL(SIGGAN_E_INVALID, "bad batch / pixel count");
    if (!isfinite(threshold)) return FAIL(SIGGAN_E_INVALID, "threshold must be finite");
    if (reinterpret_cast<uintptr_t>(x_dev) & 3) return FAIL(SIGGAN_E_INVALID, "x_dev must be 4-byte aligned");
    if ((int64_t)batch * image_stats_chunks(pixels) > INT32_MAX) return FAIL(SIGGAN_E_INVALID, "batch too large for one launch");
    DevGuard dg_(device); HIPCHK(dg_.err);
    launch_image_stats(x_dev, batch, pixels, threshold, stats_dev, (hipStream_t)stream);
    LAUNCHCHK();
    return SIGGAN_OK;
}

extern "C" int siggan_op_randn(siggan_ctx* c, float* out_dev, int64_t n, void* stream) {
    if (!c || !out_dev || n < 1) return FAIL(SIGGAN_E_INVALID, "bad argument");
    DevGuard dg_(c->cfg.device); HIPCHK(dg_.err);
    hipStream_t s = (hipStream_t)stream;
    launch_tick(c->dev, s);
    launch_randn(out_dev, n, c->dev, 3, s);
    LAUNCHCHK();
    return SIGGAN_OK;
}
