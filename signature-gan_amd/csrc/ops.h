// ops.h -- the bandwidth-bound kernels around the MFMA GEMMs (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "act.h"

namespace siggan {

// device-resident per-call state: nothing a captured launch needs lives in kernel arguments
struct DevState {
    unsigned long long seed;
    unsigned long long rng_ctr;      // + 1 per optimiser update, siggan_op_randn and mask-less training siggan_d_forward
    // scalars of the pending Adam apply (written by k_adam_prepare)
    float step_size;                 // lr / (1 - beta1^t)
    float bc2_sqrt;                  // sqrt(1 - beta2^t)
    float grad_mul;                  // grad_scale * clip coefficient
    float grad_norm;                 // pre-clip global L2 norm (after grad_scale)
    float sumsq;                     // scratch of the norm reduction
    int skip;                        // the pending update is skipped (fp16: the gradient arena holds an inf / NaN)
    float pad[2];
};

// ---- RNG (Philox4x32-10, counter = (index, stream, call counter)) --------------------------
void launch_randn(float* out, int64_t n, const DevState* st, uint32_t stream_id, hipStream_t s);
// dropout multiplier tables (0 or 1/keep) of several blocks in one launch: table t = elements [elem0[t], elem0[t] + n[t])
// (elem0 % 4 == 0) of stream sid[t], drawn at counter rng_ctr + ctr_add
void launch_dropnoise_multi(int nt, float* const* out, const int64_t* n, const int64_t* elem0, const uint32_t* sid, float keep,
                            const DevState* st, hipStream_t s, uint32_t ctr_add = 0);
// out = mask * (1/keep)
void launch_mask_to_noise(const float* mask, float* out, int64_t n, float keep, hipStream_t s);
void launch_tick(DevState* st, hipStream_t s);

// ---- fused "prepare" pass: every weight re-pack / BN-eval fold of one network in ONE launch -----
enum PrepType : int { PREP_PACK_DOWN = 0, PREP_PACK_UP, PREP_FC_T, PREP_CLS, PREP_BN_EVAL, PREP_SCALE, PREP_TAPS };
struct PrepJob {
    int type, O, I, perm;        // PACK_*: (O,I) channel counts; FC_T: O=K, I=C0; CLS: O=C; BN_EVAL: O=C, perm=perm_c0
    int dt;                      // PACK_DOWN / PACK_UP: element type of dst (DT_F32 / DT_BF16 / DT_F16); fp32 for the rest
    const float* mul;            // PACK_* / CLS / SCALE: optional device scalar every weight is multiplied by (1 / sigma of a
                                 // spectrally normalised layer); SCALE: dst[i] = src[i] * mul over O elements (fp32 copy)
    const float* src;            // weights (torch layout) / gamma
    const float* src2;           // beta
    const float* src3;           // running_mean
    const float* src4;           // running_var
    float* dst;
};
struct PrepTable {
    static constexpr int MAXJ = 32;
    int njobs;
    int overflow;                // set by prep_add when a job did not fit: launch_prepare then fails instead of dropping it
    long long prefix[MAXJ + 1];  // prefix sums of the jobs' unit (workgroup) counts
    PrepJob job[MAXJ];
};
void prep_add(PrepTable& t, const PrepJob& j);
bool launch_prepare(const PrepTable& t, float bn_eps, hipStream_t s);   // false: the table overflowed (nothing launched)
// the same plus a first-Discriminator-block forward (no dropout table) of B images, as further blocks of the one launch
bool launch_prepare_conv1(const PrepTable& t, float bn_eps, int dt, const float* x, const float* W, const float* b, float slope,
                          void* out, int B, int S, hipStream_t s);

// ---- Generator pieces ---------------------------------------------------------------------
// y[n][f'] = z[n,:] . W[f,:] + b[f],  f' = hw*C0 + c  <->  f = c*16 + hw   (NHWC feature order)
// bn_affine_relu != nullptr (eval): y = g_act((z.Wt + b) * scale + shift, gslope) with [scale | shift] of the folded BatchNorm1d.
// gslope (here and below): the Generator's activation slope, 0 = ReLU, > 0 = LeakyReLU (g_act / g_dact, act.h).
// z == nullptr: z ~ N(0,1) is drawn inside the kernel (the values launch_randn(z_out, B*K, st, stream_id) would write) and
// also stored to z_out
// (dt: element type of the activation / gradient tensors passed as void*, see act.h)
void launch_fc_fwd(int dt, const float* z, const float* Wt, const float* b, void* y, int B, int K, int C0, float gslope,
                   hipStream_t s, const float* bn_affine_relu = nullptr, const DevState* st = nullptr, uint32_t stream_id = 0,
                   float* z_out = nullptr);
// fc.hip: Linear + BatchNorm1d + activation in ONE launch on the fp32 matrix cores.  bne != nullptr: eval mode (folded [scale | shift]
// table, only `a` is written); else training: y (pre-BN), a, the bn table [scale | shift | mean | rstd | . | .] the backward
// reuses, and the running statistics / batch counter are written.  W is the torch-layout weight (no transposed copy).
// Returns false (nothing launched) when the shape is outside what the kernel covers (B > 256, or RNG draw with K % 4 != 0).
bool launch_fc_fwd_fused(int dt, const float* z, const float* W, const float* bias, void* y, void* a, const float* gamma,
                         const float* beta, float* rmean, float* rvar, int64_t* batches, float* bn, const float* bne,
                         float* z_out, const DevState* st, uint32_t sid, int B, int K, int C0, float momentum, float eps,
                         float gslope, hipStream_t s);
// activation mask + BatchNorm1d backward + dW / db of the Linear in ONE launch: da, y element type dt; dW, db, dgamma, dbeta fp32 (torch order)
bool launch_fc_bwd_fused(int dt, const void* da, const void* y, const float* z, float* bn, float* dW, float* db, float* dgamma,
                         float* dbeta, int B, int K, int C0, float gslope, hipStream_t s);
// dW[f][k] = sum_n dy[n][f'] z[n][k];  db[f] = sum_n dy[n][f']
void launch_fc_wgrad(int dt, const void* dy, const float* z, float* dW, float* db, int B, int K, int C0, hipStream_t s);

// training statistics over R rows + running-stat update (momentum, unbiased var) + batches++
void launch_bn_train_stats(int dt, const void* y, int64_t R, int C, const float* gamma, const float* beta,
                           float* rmean, float* rvar, int64_t* batches, float* bn, float* partial,
                           int perm_c0, float momentum, float eps, hipStream_t s);
// a = g_act(y*scale + shift, gslope)
void launch_bn_relu(int dt, const void* y, void* a, int64_t R, int C, const float* bn, float gslope, hipStream_t s);
// backward through g_act(BN(y)): da (in) -> dy (in place); dgamma/dbeta (torch order) written.  The activation mask is
// re-derived from y and the layer's scale/shift (the forward's own expression), so the activation is not read.
void launch_bn_bwd(int dt, void* da, const void* y, int64_t R, int C, float* bn, float* partial,
                   float* dgamma, float* dbeta, int perm_c0, float gslope, hipStream_t s, int pre_rows = 0, hipEvent_t done = nullptr);

// final 3x3 conv (C->1) + tanh, and its backward pieces.  act: [B][S][S][C] NHWC, img [B][S][S].
// bn != nullptr (training): `act` is the last block's PRE-BatchNorm tensor y and bn its [scale | shift] table -- the
// activation g_act(fma(y, scale, shift), gslope) is formed on load and never stored
// u8 != nullptr (eval only, bn == nullptr): the pass ends in k_final_fwd_u8 -- u8 [B][S][S] bytes by the reference's
// quantisation rule, stats [B][SIGGAN_IS_COUNT] int32 stroke counters against thr (optional, zeroed here), img optional
void launch_final_fwd(int dt, const void* act, const float* Wt, const float* b, float* img, int B, int S, int C, float gslope,
                      hipStream_t s, const float* bn = nullptr, hipEvent_t done = nullptr, uint8_t* u8 = nullptr,
                      int32_t* stats = nullptr, float thr = 0.f);
// backward of the last Generator block from dpre.  (1) launch_final_bwd_reduce: ONE read of y gives the BatchNorm-backward sums
// (d(act) of the final conv recomputed from dpre, never stored; activation mask re-derived from y) into `partial` AND the partial
// rows of the final conv's weight / bias gradient (activation re-derived from y) into `partial_w`;  (2) launch_final_bn_bwd_apply:
// ONE finalizer launch (dW / db from partial_w, dgamma / dbeta and the two means from `partial`), then dy
void launch_final_bwd_reduce(int dt, const float* dpre, const float* Wt, const void* y, int B, int S, int C, const float* bn,
                             float* partial, float* partial_w, float gslope, hipStream_t s);
void launch_final_bn_bwd_apply(int dt, const float* dpre, const float* Wt, const void* y, void* dy, int B, int S, int C, float* bn,
                               const float* partial, const float* partial_w, float* dW, float* db, float* dgamma, float* dbeta,
                               float gslope, hipStream_t s, hipEvent_t done = nullptr);

// ---- latent-space projection (latent.hip): eval-mode d(loss)/dz of a per-image reconstruction loss, fp32 tensors only -------
// per-image partial sums of (x - t)^2 and dpre = (2 / S^2) (x - t) (1 - x^2) from the stored fp32 image x [B][S][S]; the target
// is t_u8 (bytes through the 256-entry table lut) or t_f32, exactly one of them.  One partial per 1024 pixels:
// part[b * (S*S/1024) + j], each a fixed shuffle / LDS tree (recon_loss_parts(S) of them per image).
int recon_loss_parts(int S);
// wr / onto_dpre (siggan_g_latent_objective_grad): dpre = wr * (the above), or, onto_dpre, dpre = fmaf(wr, the above, dpre).
void launch_recon_loss(const float* img, const uint8_t* t_u8, const float* t_f32, const float* lut, float* dpre, float* part,
                       int B, int S, hipStream_t s, float wr = 1.0f, bool onto_dpre = false);
// a caller's image-space gradient `seed` (B, S, S) as a further seed: dpre = seed * (1 - img^2), or, onto_dpre, fmaf(seed, 1 - img^2, dpre)
void launch_seed_dpre(const float* img, const float* seed, float* dpre, int B, int S, bool onto_dpre, hipStream_t s);
// ONE launch for the two small jobs behind it: the per-image copies tab[b][c] = scale[c] of nt eval-mode BatchNorm scale rows
// (what EPI_LRELU_BWD multiplies by as its [B][C] table), and objective[b] = wr * recon + wd * realism + wp * prior (in that
// order; a weight of 0 leaves its term out and unread) with, optionally, terms[3][B].  recon = (part[b][0] + part[b][1] + ...)
// * inv_pixels in index order, realism[b] as given, prior = 0.5 * mean_k z[b][k]^2 (one wave per image)
struct ScaleTiles { static constexpr int MAXT = 8; int nt; const float* src[MAXT]; float* dst[MAXT]; int C[MAXT]; };
struct ObjFin { const float* part; int nparts; float inv_pixels; const float* realism; const float* z; int K; float wr, wd, wp;
                float* objective; float* terms; };
void launch_obj_fin_tiles(const ObjFin& q, int B, const ScaleTiles& t, hipStream_t s);
// eval-mode input-gradient of the final 3x3 conv through the last block's activation and folded BatchNorm:
// da[n][y][x][c] = g_dact(a[n][y][x][c]) * scale[c] * sum_{kh,kw} dpre[n][y+1-kh][x+1-kw] * Wt[kh*3+kw][c]   (C == 32)
void launch_final_dgrad_eval(const float* dpre, const float* Wt, const float* a, const float* scale, float* da, int B, int S,
                             float gslope, hipStream_t s);
// dz[b][k] = sum_f' dh[b][f'] * g_dact(a0[b][f']) * scale0[f'] * W[f(f')][k], f' = hw*C0 + c <-> f = c*16 + hw (W: the torch-layout
// (F, K) fc weight).  F is split over workgroups; the partial rows land in `part` (part_cap floats) and are added in split order.
// Any K >= 1.
void launch_fc_dz(const float* dh, const float* a0, const float* scale0, const float* W, float* dz, float* part, int64_t part_cap,
                  int B, int K, int C0, float gslope, hipStream_t s, const float* z = nullptr, float wpl = 0.f);   // z: dz += wpl * z
void launch_prior_dz(const float* z, float* dz, int64_t n, float wpl, hipStream_t s);       // dz = wpl * z

// ---- eval-mode parameter gradient (paramgrad.hip): what siggan_g_param_grad adds to the pieces above, fp32 tensors only ------
// BatchNorm as the fixed affine of eval mode.  g [R][C]: dpost = d(activation output) * act' in, dy = scale[c] * dpost out (in
// place); y [R][C] the block's PRE-BatchNorm output; bne the eval table [scale | shift | mean | rstd].  dbeta[c] = sum dpost,
// dgamma[c] = sum dpost * (y - mean) * rstd (right for gamma of either sign and for gamma == 0), two launches, fixed order.
// false (nothing launched): a channel count the kernel does not cover.
bool launch_bn_eval_bwd(float* g, const float* y, int64_t R, int C, const float* bne, float* part, int64_t part_cap,
                        float* dgamma, float* dbeta, hipStream_t s);
// the final 3x3 conv's dW (torch order [c][kh][kw], C == 32) and db from dpre and the stored last activation a [B][S][S][32];
// two launches, `part` holds one row of 289 floats per workgroup.  false (nothing launched): part_cap cannot hold them.
bool launch_final_wgrad_eval(const float* dpre, const float* a, float* part, int64_t part_cap, float* dW, float* db, int B, int S,
                             hipStream_t s);
// the fc block: dh [B][F] (NHWC feature order f') = d(activation output) in, scale0[f'] * g_dact(a0) * dh out (in place: what
// launch_fc_wgrad takes as dy); dgamma / dbeta of the BatchNorm1d in torch order, xhat from z . W + bias formed again
void launch_fc_bn_eval_bwd(float* dh, const float* a0, const float* bne, const float* W, const float* bias, const float* z,
                           float* dgamma, float* dbeta, int B, int K, int C0, float gslope, hipStream_t s);
// g[i] = g[i] + weight * (p[i] - p0[i]), i < n: the gradient of 0.5 * weight * |p - p0|^2 added onto g (siggan_op_anchor)
void launch_anchor(float* g, const float* p, const float* p0, int64_t n, float weight, hipStream_t s);

// ---- Discriminator pieces -----------------------------------------------------------------
// first block (Cin = 1): x = two segments (x0: n < n0, x1: the rest), out [B][S/2][S/2][C]
void launch_conv1_fwd(int dt, const float* x0, int n0, const float* x1, const float* W, const float* b,
                      const float* noise, float slope, void* out, int B, int S, int C, hipStream_t s);
// the same block from bytes (eval mode, no dropout): u8 (B,S,S), binarize -1 (off) or 0..255 (b < binarize ? 0 : 255 first),
// lut[256] the dequantised value of each byte, x_out optional (B,1,S,S) fp32: the tensor the block was fed
struct Conv1U8 { const uint8_t* u8; const float* lut; float* x_out; int binarize; };
void launch_conv1_fwd_u8(int dt, const Conv1U8& u, const float* W, const float* b, float slope, void* out, int B, int S, int C,
                         hipStream_t s);
void launch_conv1_wgrad(int dt, const void* dv, const float* x0, int n0, const float* x1, float* dW, float* db,
                        float* partial, int B, int S, int C, hipStream_t s);
// d(image) = conv1 input-gradient, times tanh' = 1 - img^2  ->  dpre
void launch_conv1_dgrad_tanh(int dt, const void* dv, const float* Wt, const float* img, float* dpre, int B, int S,
                             int C, hipStream_t s);
void launch_cls_fwd(int dt, const void* act, const float* wcp, const float* bc, float* logits, int B, int F, hipStream_t s);
void launch_cls_features(int dt, const void* act, float* feat, int B, int C, hipStream_t s);
// sigmoid + BCE (mean per segment) + d(logit); seg0 = first n0 rows with target y0, rest target y1
// gscale: d(logit) is multiplied by it (the fp16 gradient scale; every gradient downstream then carries it and the optimiser
// step divides it out again -- 1 for fp32 / bf16)
// The logit of row n: stored (k_cls_fwd; P == 0, logits alone), or -- when the last block's split-K epilogue left P partial dot
// products per image (GConvArgs::cls_part) -- their sum in order plus the bias bc[0]; `logits` then receives the sum (k_bce).
struct LogitSrc { const float* logits; const float* parts; int P; const float* bc; };
void launch_bce(const LogitSrc& src, int B, int n0, float y0, float y1, float* probs, float* dlogit, float* metrics, int is_g_step,
                hipStream_t s, float gscale = 1.0f);
// dv[n][hw][c] = dlogit[n] * wcp[hw*C+c] * leaky'(act) * noise[n][c]
// from the logits (rows < n0: target y0, the rest y1; each segment's mean): d(logit) is recomputed with k_bce's expression
// bce != nullptr: launch_bce's work (same rows, targets and gscale) rides as one more block of this launch
struct BceRider { float* probs; float* dlogit; float* metrics; int is_g; };
void launch_cls_bwd(int dt, const LogitSrc& src, int n0, float y0, float y1, const float* wcp, const void* act, const float* noise,
                    float slope, void* dv, int B, int C, hipStream_t s, float gscale = 1.0f, const BceRider* bce = nullptr);
// the same in eval form, per image (siggan_g_latent_objective_grad; fp32): no dropout table, target 1 with a count of 1,
// d(logit) times wd;  term[n] = -max(log p[n], -100) and (optional) probs[n] = p[n] are written by one more block
void launch_cls_bwd_eval(const LogitSrc& src, const float* wcp, const float* act, float slope, float* dv, int B, int C, float wd,
                         float* term, float* probs, hipStream_t s);
// dWc (torch order c*16+hw) and dbc
void launch_cls_wgrad(int dt, const float* dlogit, const void* act, float* dWc, float* dbc, int B, int C, hipStream_t s);
// dst[i] = (float)src[i] for a tensor of element type dt
void launch_to_f32(int dt, const void* src, float* dst, int64_t n, hipStream_t s);

// ---- spectral normalisation of the Discriminator (sn.hip) -------------------------------------------------------------
struct SnLayer {
    const float* W;              // weight_orig in the parameter arena, (rows, K) row-major = weight.view(Cout, -1)
    int rows, K;
    int u_off, v_off;            // offsets of this layer's u / v inside the flat u / v arenas (and of tbuf / wbuf)
    int64_t w_off;               // offset of the weight tensor inside the gradient arena
};
struct SnTable {
    static constexpr int MAXS = 8;          // conv blocks + classifier
    int n;
    SnLayer layer[MAXS];
    int pre_k[MAXS + 1], pre_r[MAXS + 1];   // prefix sums of ceil(K / 256) and ceil(rows / 4): workgroups of k_sn_wtu / k_sn_wv
    float *u, *v;                           // the caller's weight_u / weight_v buffers (flat, layer order)
    float *tbuf, *wbuf;                     // scratch: W^T u (v-sized), W v (u-sized)
    float* sig;                             // [3 slots][sigma | 1/sigma][MAXS]
    float *u_saved, *v_saved;               // [3 slots][u_total] / [3 slots][v_total]: each pass's (u, v)
    float* dots;                            // [2 passes][MAXS][64] partial <G_p, W>
    int u_total, v_total;
    int slot[2];                            // k_sn_combine: the sigma slot of pass 0 / pass 1
};
// sigma (+ one power iteration when training) of every layer for one pass, results into slot
void launch_sn_sigma(const SnTable& t, int training, int slot, float eps, hipStream_t s);
// out[arena] = sum over passes of the gradient w.r.t. weight_orig (through sigma) from the per-pass gradients w.r.t. the
// normalised weights g0 / g1 (whole-arena temporaries; non-weight entries are added plainly)
void launch_sn_combine(const SnTable& t, const float* g0, const float* g1, float* out, int64_t total, int npass, hipStream_t s);

// ---- optimiser ------------------------------------------------------------------------------
// launch_grad_sumsq: per-block partial sums of squares of the arena into `partial` (512 floats); whoever needs the norm adds
// them itself in one fixed order (k_adam_prepare when handed `sumsq_partial`, every block of the fused k_adam): no finalize launch.
// launch_adam_prepare: reads steps[0], writes steps[i] += 1 for every tensor, derives the Adam scalars; with clip_max_norm > 0
// (or check_finite) it needs launch_grad_sumsq first and its `partial` as sumsq_partial
void launch_grad_sumsq(const float* g, int64_t n, float* partial, hipStream_t s);
// check_finite (fp16 chains; needs launch_grad_sumsq first): a non-finite sum of squares marks the update as skipped
// (DevState::skip: k_adam returns at once, the step counts stay) and writes 1 to *metric_skipped, else 0
void launch_adam_prepare(DevState* st, float* steps, int ntensors, double lr, double beta1, double beta2,
                         float grad_scale, float clip_max_norm, float* metric_norm, hipStream_t s,
                         int check_finite = 0, float* metric_skipped = nullptr, const float* sumsq_partial = nullptr);
// beta^t for an integer-valued step count by repeated squaring in double: the SAME arithmetic on the host (fused path below)
// and on the device (k_adam_prepare), so the two paths give bit-identical bias corrections (within an ulp of libm's pow,
// which torch's Python-side `beta ** step` uses)
__host__ __device__ inline double pow_step(double b, double t) {
    unsigned long long n = (unsigned long long)t;
    double r = 1.0;
    while (n) { if (n & 1) r *= b; b *= b; n >>= 1; }
    return r;
}
// One-launch optimiser update (no k_adam_prepare in front): the caller knows the step count `t` (AFTER the increment) on the
// host and passes the bias-corrected scalars; the kernel derives the clip coefficient from DevState::sumsq itself, block 0
// writes steps[0..ntensors) = t, ticks the RNG epoch and stores the pre-clip norm.  Same update arithmetic as launch_adam.
void launch_adam_fused(float* p, float* g, float* m, float* v, int64_t n, DevState* st, float* steps, int ntensors, double t,
                       double lr, double beta1, double beta2, double eps, float grad_scale, float clip_max_norm,
                       float* metric_norm, const float* sumsq_partial, hipStream_t s, float* metric_skipped = nullptr);
void launch_adam(float* p, float* g, float* m, float* v, int64_t n, const DevState* st, double beta1,
                 double beta2, double eps, int write_back_grad, hipStream_t s);

// ---- the one-launch update that also rebuilds what the next pass derives from the arena ------------------------------
// launch_adam_fused plus launch_prepare's work in ONE launch: the arena is covered by a job table; a workgroup that owns a
// 16 x 16 x 16-tap tile of a convolution weight updates it and writes both MFMA packs from LDS (64-byte runs each way), the
// classifier / one-channel weights and the BatchNorm eval tables likewise.  Same update arithmetic, same pack values as the
// two launches it replaces (bitwise: tests/test_engine_gpu.py compares the execution modes).  Both job tables are built from
// one list of records (ctx.h, struct Derived: which fields mean what is said there, once); the destination layouts are
// the functions both kernels call (ops.hip, pack_down_idx / pack_up_idx / bn_eval_store).
enum ApType : int { AP_FLAT = 0, AP_CONV, AP_T16, AP_TAPS, AP_BN };
struct ApJob {
    int type;
    int A, Bc, dt;               // as in the record (BN: Bc = perm_c0)
    long long off, n;            // first arena element, element count (FLAT / TAPS; the other types know it from A, Bc)
    long long off2, n2;          // TAPS: a second flat range owned by the same workgroup (the layer's bias); BN: off2 = beta
    float* dst;                  // CONV: the down pack; T16 / TAPS: the permuted copy; BN: the table
    float* dst2;                 // CONV: the up pack
    const float* rmean;          // BN: running statistics
    const float* rvar;
    int wait;                    // TAPS: riders that must have read this job's ranges before it writes them (ApRide), 0: none
};
struct ApTable {
    static constexpr int MAXJ = 24;
    int njobs, overflow;
    long long prefix[MAXJ + 1];  // prefix sums of the jobs' workgroup counts
    ApJob job[MAXJ];
};
void ap_add(ApTable& t, const ApJob& j);
// Riders: further workgroups of the same launch run the first Discriminator block's forward of B images with the block's
// UPDATED weights, which each of them derives for itself from the arena (1088 values); the workgroup that owns those ranges
// writes them only after every rider has read them (`counter`: one zero-initialised word, left at zero).  If the owner's wait
// is bounded out before every rider has reported, it still takes the whole launch's count off `counter` (the late riders bring
// it back to zero) and sets `late` (a sticky word of host-visible memory: the step's caller is told, siggan.hip lane_check).
struct ApRide { const float* x; void* out; int B, S, dt; float slope; long long w_off, b_off; unsigned* counter; unsigned* late; };
bool launch_adam_pack(const ApTable& t, float* p, float* g, float* m, float* v, DevState* st, float* steps, int ntensors,
                      double tstep, double lr, double beta1, double beta2, double eps, float grad_scale, float clip_max_norm,
                      float* metric_norm, const float* sumsq_partial, float* metric_skipped, float bn_eps,
                      const ApRide* ride, hipStream_t s);

// input pipeline: out[b] = lut[ resample(cache[index[b]]) ], (B,1,S,S) fp32 from an (N,S,S) uint8 cache (see k_augment)
void launch_augment(const uint8_t* cache, int64_t n_images, const int32_t* index, const int32_t* prm, const int16_t* tabs,
                    const float* lut, float* out, int B, int S, int augment, int fill, hipStream_t s);

// stats [B][SIGGAN_IS_COUNT] int32 (zeroed here): per-image stroke counters of x [B][P] fp32 against thr (see k_image_stats)
int image_stats_chunks(int64_t P);
void launch_image_stats(const float* x, int B, int64_t P, float thr, int32_t* stats, hipStream_t s);

}  // namespace siggan
