// latent.hip -- the kernels of siggan_g_latent_objective_grad (and siggan_g_latent_grad, its reconstruction-only case) that the
// training step does not already have (gfx950, fp32 tensors): the per-image reconstruction loss with d(pre-tanh), the objective
// with the per-image scale tables the implicit-GEMM epilogue EPI_LRELU_BWD multiplies by, the final conv's input-gradient in
// eval form, and the fc layer's input-gradient dz = dh . W.
//
// Every sum has a fixed order (shuffle tree inside a wave, index order across waves, workgroups and splits) and nothing is
// accumulated with atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include "ops.h"

namespace siggan {

typedef f32x4 f4v;
__device__ __forceinline__ f4v ldg4(const float* p) { return *reinterpret_cast<const f4v*>(p); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// =========================================================================================
// loss: 256 threads x 4 pixels = 1024 pixels of ONE image per workgroup (S*S is a multiple of 1024)
//   d = x - t,  dpre = ((2 / S^2) * d) * (1 - x * x),  part[workgroup] = sum d^2
// The byte route reads t from the 256-entry table, the fp32 route reads it as given: the same t gives the same bits.
// MODE (siggan_g_latent_objective_grad): 0 dpre as above; 1 dpre = wr * (the above); 2 dpre = fmaf(wr, the above, dpre) -- the
// Discriminator's d(pre-tanh) is already there (k_conv1_dgrad_tanh) and the two seeds meet here, each element read and written
// by its own thread.  wr = 1 in mode 1 would give mode 0's bits (a multiplication by 1 is exact); the host picks mode 0 for it.
// =========================================================================================
int recon_loss_parts(int S) { return S * S / 1024; }

template <bool U8, int MODE>
__global__ __launch_bounds__(256) void k_recon_loss(const float* __restrict__ img, const uint8_t* __restrict__ tu,
                                                    const float* __restrict__ tf, const float* __restrict__ lut,
                                                    float* __restrict__ dpre, float* __restrict__ part, float c2, float wr) {
    __shared__ float sh[4];
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const f4v x = ldg4(img + i);
    f4v t;
    if (U8) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(tu + i);
        t = f4v{lut[w & 255u], lut[(w >> 8) & 255u], lut[(w >> 16) & 255u], lut[w >> 24]};
    } else {
        t = ldg4(tf + i);
    }
    f4v o;
    if (MODE == 2) o = ldg4(dpre + i);
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = x[e] - t[e];
        const float r = (c2 * d) * (1.0f - x[e] * x[e]);
        o[e] = MODE == 0 ? r : (MODE == 1 ? wr * r : fmaf(wr, r, o[e]));
        ss += d * d;
    }
    *reinterpret_cast<f4v*>(dpre + i) = o;
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) ss += __shfl_down(ss, k, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

void launch_recon_loss(const float* img, const uint8_t* t_u8, const float* t_f32, const float* lut, float* dpre, float* part,
                       int B, int S, hipStream_t s, float wr, bool onto_dpre) {
    const float c2 = 2.0f / (float)(S * S);              // a power of two (S = 64, 128): exact
    const dim3 grid((unsigned)(B * recon_loss_parts(S)));
    const int mode = onto_dpre ? 2 : (wr == 1.0f ? 0 : 1);
#define SIGGAN_RECON(U8, MODE) hipLaunchKernelGGL((k_recon_loss<U8, MODE>), grid, dim3(256), 0, s, img, t_u8, t_f32, lut, dpre, part, c2, wr)
    if (t_u8) { if (mode == 0) SIGGAN_RECON(true, 0); else if (mode == 1) SIGGAN_RECON(true, 1); else SIGGAN_RECON(true, 2); }
    else      { if (mode == 0) SIGGAN_RECON(false, 0); else if (mode == 1) SIGGAN_RECON(false, 1); else SIGGAN_RECON(false, 2); }
#undef SIGGAN_RECON
}

// =========================================================================================
// a caller-supplied image-space gradient (siggan_g_latent_objective_grad_seeded) joins the seeds of d(pre-tanh):
// dpre = fmaf(seed, 1 - x * x, dpre) behind the Discriminator's and the reconstruction's, or seed * (1 - x * x) when nothing is
// there yet.  Four pixels per thread, each element read and written by its own thread.
// =========================================================================================
template <bool ONTO>
__global__ __launch_bounds__(256) void k_seed_dpre(const float* __restrict__ img, const float* __restrict__ seed,
                                                   float* __restrict__ dpre) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const f4v x = ldg4(img + i), g = ldg4(seed + i);
    f4v o;
    if (ONTO) o = ldg4(dpre + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = 1.0f - x[e] * x[e];
        o[e] = ONTO ? fmaf(g[e], t, o[e]) : g[e] * t;
    }
    *reinterpret_cast<f4v*>(dpre + i) = o;
}

void launch_seed_dpre(const float* img, const float* seed, float* dpre, int B, int S, bool onto_dpre, hipStream_t s) {
    const dim3 grid((unsigned)(B * (S * S / 1024)));
    if (onto_dpre) hipLaunchKernelGGL(k_seed_dpre<true>, grid, dim3(256), 0, s, img, seed, dpre);
    else hipLaunchKernelGGL(k_seed_dpre<false>, grid, dim3(256), 0, s, img, seed, dpre);
}

// =========================================================================================
// the objective and the per-image scale tables, one launch: workgroups [0, nbl) finish the OBJECTIVE, one wave per image (four
// images per workgroup), the rest copy tile t's scale row once per image (a float4 per thread).  recon: the loss partials in
// index order, times 1 / S^2 (every lane forms the same sum).  prior 0.5 * mean_k z^2: lane j adds z[j]^2, z[j + 64]^2, ... in
// index order, then the shuffle tree.  The realism term was written by k_cls_bwd_eval.  A term whose weight is 0 is not read and
// counts (and is reported) as 0; with the weights (1, 0, 0) the objective is the recon term's bits (0 + 1 * recon).
// =========================================================================================
struct TileLaunch { ScaleTiles t; int prefix[ScaleTiles::MAXT + 1]; };

__device__ __forceinline__ void copy_tile_block(const TileLaunch& tl, int bid, int B) {
    int t = 0;
    while (t + 1 < tl.t.nt && bid >= tl.prefix[t + 1]) ++t;
    const int C4 = tl.t.C[t] / 4;
    const int64_t i4 = (int64_t)(bid - tl.prefix[t]) * 256 + threadIdx.x;
    if (i4 >= (int64_t)B * C4) return;
    const int c4 = (int)(i4 % C4);
    *reinterpret_cast<f4v*>(tl.t.dst[t] + i4 * 4) = ldg4(tl.t.src[t] + c4 * 4);
}

__global__ __launch_bounds__(256) void k_obj_fin_tiles(const ObjFin q, int B, int nbl, const TileLaunch tl) {
    const int bid = blockIdx.x;
    if (bid >= nbl) { copy_tile_block(tl, bid - nbl, B); return; }
    const int lane = threadIdx.x & 63, b = bid * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                  // (a whole wave: the shuffles below see all 64 lanes)
    float recon = 0.f, real = 0.f, prior = 0.f, obj = 0.f;
    if (q.wr > 0.f) {
        float s = q.part[(size_t)b * q.nparts];
        for (int j = 1; j < q.nparts; ++j) s += q.part[(size_t)b * q.nparts + j];
        recon = s * q.inv_pixels;
        obj += q.wr * recon;
    }
    if (q.wd > 0.f) { real = q.realism[b]; obj += q.wd * real; }
    if (q.wp > 0.f) {
        float s = 0.f;
        for (int k = lane; k < q.K; k += 64) { const float v = q.z[(size_t)b * q.K + k]; s = fmaf(v, v, s); }
#pragma unroll
        for (int k = 32; k > 0; k >>= 1) s += __shfl_xor(s, k, 64);
        prior = 0.5f * (s / (float)q.K);
        obj += q.wp * prior;
    }
    if (lane == 0) {
        q.objective[b] = obj;
        if (q.terms) { q.terms[b] = recon; q.terms[B + b] = real; q.terms[2 * (size_t)B + b] = prior; }
    }
}

void launch_obj_fin_tiles(const ObjFin& q, int B, const ScaleTiles& t, hipStream_t s) {
    TileLaunch tl; tl.t = t; tl.prefix[0] = 0;
    for (int i = 0; i < t.nt; ++i) tl.prefix[i + 1] = tl.prefix[i] + cdiv((int64_t)B * (t.C[i] / 4), 256);
    const int nbl = cdiv(B, 4);
    hipLaunchKernelGGL(k_obj_fin_tiles, dim3((unsigned)(nbl + tl.prefix[t.nt])), dim3(256), 0, s, q, B, nbl, tl);
}

// =========================================================================================
// final 3x3 conv (32 -> 1), input-gradient in eval form.  The layout of the training path's strip kernels (ops.hip,
// k_final_bnbwd_apply): 8 lanes per pixel (4 channels each, the nine taps' weights in registers) x 32 pixels along a row, a
// workgroup owns a 4-row strip of one image and reads its (4 + 2) x 34 dpre neighbourhood (zero outside the image) through LDS.
// Here the activation mask comes from the STORED activation and the BatchNorm is its eval-mode per-channel scale.
// =========================================================================================
template <bool LK>
__global__ __launch_bounds__(256) void k_final_dgrad_eval(const float* __restrict__ dpre, const float* __restrict__ Wt,
                                                          const float* __restrict__ a, const float* __restrict__ scale,
                                                          float* __restrict__ da, int S, float gs) {
    constexpr int RY = 4, C = 32, PW = 34;
    __shared__ float sp[(RY + 2) * PW];
    const int c4 = threadIdx.x & 7, xi = threadIdx.x >> 3;
    const int nbx = S >> 5, nby = S / RY;
    int sid = blockIdx.x;
    const int xb = (sid % nbx) * 32; sid /= nbx;
    const int y0 = (sid % nby) * RY, n = sid / nby;
    f4v w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = ldg4(Wt + k * 32 + c4 * 4);
    const f4v sc = ldg4(scale + c4 * 4);
    if (threadIdx.x < (RY + 2) * PW) {
        const int r = threadIdx.x / PW, k = threadIdx.x - r * PW;
        const int yy = y0 + r - 1, xx = xb + k - 1, yc = clampi(yy, S - 1), xc = clampi(xx, S - 1);
        const float q = dpre[((size_t)n * S + yc) * S + xc];
        sp[threadIdx.x] = (yy == yc && xx == xc) ? q : 0.f;
    }
    const size_t o0 = (((size_t)n * S + y0) * S + xb + xi) * C + c4 * 4;
    f4v av[RY];
#pragma unroll
    for (int r = 0; r < RY; ++r) av[r] = ldg4(a + o0 + (size_t)r * S * C);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RY; ++r) {
        f4v g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const float d = sp[(r + 2 - kh) * PW + xi + 2 - kw];       // dpre[y + 1 - kh][x + 1 - kw]
                const f4v ww = w[kh * 3 + kw];
                g.x = fmaf(d, ww.x, g.x); g.y = fmaf(d, ww.y, g.y); g.z = fmaf(d, ww.z, g.z); g.w = fmaf(d, ww.w, g.w);
            }
        const f4v v = av[r];
        f4v o;
        o.x = g_dact<LK>(v.x, g.x, gs) * sc.x; o.y = g_dact<LK>(v.y, g.y, gs) * sc.y;
        o.z = g_dact<LK>(v.z, g.z, gs) * sc.z; o.w = g_dact<LK>(v.w, g.w, gs) * sc.w;
        *reinterpret_cast<f4v*>(da + o0 + (size_t)r * S * C) = o;
    }
}

void launch_final_dgrad_eval(const float* dpre, const float* Wt, const float* a, const float* scale, float* da, int B, int S,
                             float gslope, hipStream_t s) {
    const dim3 grid((unsigned)(B * (S / 4) * (S / 32)));
    SIGGAN_GS_SWITCH(gslope, LK, hipLaunchKernelGGL((k_final_dgrad_eval<LK>), grid, dim3(256), 0, s, dpre, Wt, a, scale, da, S, gslope));
}

// =========================================================================================
// fc input-gradient.  A workgroup owns FC consecutive features f' (NHWC order) of a tile of 8 images: it stages
// g[bt][f'] = g_dact(a0) * dh * scale0[f'] in LDS 64 features at a time, wave w walks 16 of them, lane = one latent index k
// (W rows are K-contiguous: coalesced), plain fp32 FMAs.  The fp32 matrix cores run at the vector rate on gfx950 and would need
// K padded to the 32-wide tile (latent 100, 50); at ~50 MFLOP the kernel is bound by launch and load latency, not by FLOPs.
// The four waves meet in LDS (wave order), the splits of F in k_fc_dz_sum (split order).
// =========================================================================================
constexpr int DZ_BT = 8, DZ_SUB = 64;        // (restated in tests/evalpaths.py, matched as text by tests/test_eval_paths_cpu.py, as are nsplit's rule in launch_fc_dz and the
                                             //  workgroup counts of launch_obj_fin_tiles / k_obj_fin_tiles)

template <bool LK>
__global__ __launch_bounds__(256) void k_fc_dz(const float* __restrict__ dh, const float* __restrict__ a0,
                                               const float* __restrict__ sc0, const float* __restrict__ W, float* __restrict__ out,
                                               int B, int K, int C0, int F, int FC, float gs) {
    __shared__ float sg[DZ_BT][DZ_SUB];
    __shared__ int srow[DZ_SUB];
    __shared__ float sacc[4][DZ_BT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.y * DZ_BT, f_begin = blockIdx.x * FC;
    float* const o = out + (size_t)blockIdx.x * B * K;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        float acc[DZ_BT];
#pragma unroll
        for (int bt = 0; bt < DZ_BT; ++bt) acc[bt] = 0.f;
        for (int f0 = f_begin; f0 < f_begin + FC; f0 += DZ_SUB) {
            __syncthreads();                                   // the previous chunk (and sacc of the previous k0) has been read
            for (int e = tid; e < DZ_BT * DZ_SUB; e += 256) {
                const int bt = e / DZ_SUB, j = e - bt * DZ_SUB, b = b0 + bt, fp = f0 + j;
                float g = 0.f;
                if (b < B) {
                    const size_t idx = (size_t)b * F + fp;
                    g = g_dact<LK>(a0[idx], dh[idx], gs) * sc0[fp];
                }
                sg[bt][j] = g;
            }
            if (tid < DZ_SUB) { const int fp = f0 + tid; srow[tid] = (fp % C0) * 16 + fp / C0; }
            __syncthreads();
            if (k < K) {
#pragma unroll 4
                for (int j = wave * 16; j < wave * 16 + 16; ++j) {
                    const float w = W[(size_t)srow[j] * K + k];
#pragma unroll
                    for (int bt = 0; bt < DZ_BT; ++bt) acc[bt] = fmaf(sg[bt][j], w, acc[bt]);
                }
            }
        }
#pragma unroll
        for (int bt = 0; bt < DZ_BT; ++bt) sacc[wave][bt][lane] = acc[bt];
        __syncthreads();
        for (int e = tid; e < DZ_BT * 64; e += 256) {
            const int bt = e >> 6, l = e & 63;
            if (b0 + bt < B && k0 + l < K)
                o[(size_t)(b0 + bt) * K + k0 + l] = ((sacc[0][bt][l] + sacc[1][bt][l]) + sacc[2][bt][l]) + sacc[3][bt][l];
        }
    }
}

// PRIOR: the prior term's gradient wpl * z[i] (wpl = prior_weight / latent) is added here, behind the ordered sum (part may be dz
// itself with nsplit 1: every thread reads and writes its own element)
template <bool PRIOR>
__global__ __launch_bounds__(256) void k_fc_dz_sum(const float* part, int nsplit, int64_t n, float* dz, const float* __restrict__ zin, float wpl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int z = 1; z < nsplit; ++z) s += part[(size_t)z * n + i];
    dz[i] = PRIOR ? fmaf(wpl, zin[i], s) : s;
}

void launch_fc_dz(const float* dh, const float* a0, const float* scale0, const float* W, float* dz, float* part, int64_t part_cap,
                  int B, int K, int C0, float gslope, hipStream_t s, const float* z, float wpl) {
    const int F = C0 * 16;                               // a multiple of DZ_SUB (C0 = 256, 512)
    const int64_t n = (int64_t)B * K;
    int nsplit = F / DZ_SUB;
    while (nsplit > 1 && (int64_t)nsplit * n > part_cap) nsplit >>= 1;     // a batch x latent the carve cannot hold split: fewer, longer splits
    float* const out = nsplit > 1 ? part : dz;
    const dim3 grid((unsigned)nsplit, (unsigned)cdiv(B, DZ_BT));
    SIGGAN_GS_SWITCH(gslope, LK, hipLaunchKernelGGL((k_fc_dz<LK>), grid, dim3(256), 0, s, dh, a0, scale0, W, out, B, K, C0, F, F / nsplit, gslope));
    const dim3 gsum((unsigned)cdiv(n, 256));
    if (z) hipLaunchKernelGGL((k_fc_dz_sum<true>), gsum, dim3(256), 0, s, out, nsplit, n, dz, z, wpl);
    else if (nsplit > 1) hipLaunchKernelGGL((k_fc_dz_sum<false>), gsum, dim3(256), 0, s, part, nsplit, n, dz, z, wpl);
}

// the objective of the prior alone: dz = wpl * z, no chain behind it
__global__ __launch_bounds__(256) void k_prior_dz(const float* __restrict__ z, float* __restrict__ dz, int64_t n, float wpl) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dz[i] = wpl * z[i];
}
void launch_prior_dz(const float* z, float* dz, int64_t n, float wpl, hipStream_t s) {
    hipLaunchKernelGGL(k_prior_dz, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, z, dz, n, wpl);
}

}  // namespace siggan
