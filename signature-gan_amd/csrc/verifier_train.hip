// verifier_train.hip -- train step of the Siamese signature verifier (include/siggan_verifier_train.h; the reference's
// signature_verifier_train.py:376-449).  gfx950 only, fp32 only, NHWC inside the library (pool3 and everything behind it in
// torch's (c, h, w) flatten order, so fc1 reads and writes the arena's fc1.weight as it is).
//
// Forward, per conv layer: the convolution WITHOUT its bias (a train-mode BatchNorm removes it again; it only enters the
// running mean) -> per-half column sums (mean, then centred sum of squares: partial rows + an ordered sum) -> one pass that
// applies BatchNorm, ReLU and the 2x2 max and writes the pooled tensor and one route byte per pooled element.
//   k_tconv1    direct 5x5 stencil (Cin = 1), fp32 or uint8 images
//   k_tconv     (verifier_parts.h) stride-1 implicit GEMM on v_mfma_f32_32x32x2_f32 (conv_tile, the one k_vconv runs; raw store): conv2 / conv3 forward and,
//               over a tap-flipped channel-transposed pack, their input gradients
//   k_tgemm     (verifier_parts.h) 64 x 64 MFMA tiles with either operand K- or M-contiguous: fc1 forward (16 K slices), dX = dY.W, dW = dY^T.X
//   k_ttail     per image row: ordered K-slice sum + bias + ReLU + dropout, fc2, L2 normalise
//   k_thead     per pair: head forward, both losses and the head's backward down to d(e1) = -d(e2)
// Backward: k_tembbwd (normalise / fc2 / dropout / ReLU per row), k_tgemm twice, then per conv layer k_bnbwd_red (scatter by
// route, per-half sums of dz and dz * xhat), k_bnbwd_apply (dy), k_twgrad (split-K MFMA GEMM over K = n * H * W into slabs)
// + k_wgrad_sum (ordered slab sum into torch's weight layout), k_tconv for the input gradient.
// No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <new>

#include "../../include/siggan_verifier_train.h"
#include "host.h"
#include "ops.h"
#include "rng.h"
#include "verifier_parts.h"

using namespace siggan;

namespace {

constexpr float P_FC = 0.5f, P_CLS = 0.3f;
constexpr uint32_t SID_FC1 = 0x56540001u, SID_FC2 = 0x56540002u, SID_CLS = 0x56540003u;   // dropout sites: fc (x1), fc (x2), classifier
constexpr float BN_MOMENTUM = 0.1f;

// keep decision of element i of a dropout site
__device__ __forceinline__ bool drawn_keep(unsigned long long seed, unsigned long long ctr, uint64_t i, uint32_t sid, float keep) {
    const uint4 r = draw_raw(seed, ctr, i >> 2, sid);
    const uint32_t x[4] = {r.x, r.y, r.z, r.w};
    return u01(x[i & 3]) < keep;
}

// ---------------------------------------------------------------- weight packs (every step: the arena moves)
// torch (Co, Ci, T) -> fwd [Co][t * Ci + ci] and, for the input gradient, flip [Ci][t' * Co + co] with t' = T - 1 - t
__global__ void k_tpack(const float* __restrict__ w, float* __restrict__ fwd, float* __restrict__ flip, int Co, int Ci, int T) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Co * Ci * T) return;
    const int t = (int)(i % T), ci = (int)((i / T) % Ci), co = (int)(i / ((int64_t)T * Ci));
    const float v = w[i];
    fwd[((int64_t)co * T + t) * Ci + ci] = v;
    flip[((int64_t)ci * T + (T - 1 - t)) * Co + co] = v;
}

// ---------------------------------------------------------------- conv1 forward (no bias): y (N, 64, 64, 32)
// thread = (pixel, 8 output channels); block = 64 pixels (one image row) x 4 channel groups
template <bool U8>
__global__ __launch_bounds__(256) void k_tconv1(const void* __restrict__ x1, const void* __restrict__ x2, int nsplit,
                                                const float* __restrict__ w /* (32, 25) */, float* __restrict__ y) {
    __shared__ float sW[25][32];
    const int tid = threadIdx.x;
    for (int i = tid; i < 800; i += 256) sW[i % 25][i / 25] = w[i];
    __syncthreads();
    const int cg = tid & 3;
    const int64_t P = (int64_t)blockIdx.x * 64 + (tid >> 2);
    const int n = (int)(P >> 12), py = (int)(P >> 6) & 63, px = (int)P & 63;
    const void* img = vimage<U8>(x1, x2, nsplit, n);
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            const int iy = py + ky - 2, ix = px + kx - 2;
            const float xv = (iy >= 0 && iy < VS && ix >= 0 && ix < VS) ? vload<U8>(img, iy * VS + ix) : 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fmaf(xv, sW[ky * 5 + kx][cg * 8 + c], acc[c]);
        }
    float* o = y + (size_t)P * 32 + cg * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = acc[c];
}

// conv1 weight gradient: block = 16 image rows (1024 pixels); thread = (channel, tap group), taps tg, tg + 8, ...
// part [N * 4][32 * 25] in torch's (co, tap) order
template <bool U8>
__global__ __launch_bounds__(256) void k_tconv1_wgrad(const void* __restrict__ x1, const void* __restrict__ x2, int nsplit,
                                                      const float* __restrict__ dy /* (N, 64, 64, 32) */, float* __restrict__ part) {
    __shared__ float sX[20][68];
    const int tid = threadIdx.x, n = blockIdx.x >> 2, band = blockIdx.x & 3;
    const void* img = vimage<U8>(x1, x2, nsplit, n);
    for (int i = tid; i < 20 * 68; i += 256) {
        const int r = i / 68, c = i % 68;
        const int iy = band * 16 + r - 2, ix = c - 2;
        sX[r][c] = (iy >= 0 && iy < VS && ix >= 0 && ix < VS) ? vload<U8>(img, iy * VS + ix) : 0.f;
    }
    __syncthreads();
    const int co = tid & 31, tg = tid >> 5;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* d = dy + ((size_t)n * 4096 + (size_t)band * 1024) * 32 + co;
    for (int p = 0; p < 1024; ++p) {
        const float g = d[(size_t)p * 32];
        const int py = p >> 6, px = p & 63;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = tg + 8 * i;
            if (t < 25) acc[i] = fmaf(g, sX[py + t / 5][px + t % 5], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = tg + 8 * i;
        if (t < 25) part[(size_t)blockIdx.x * 800 + co * 25 + t] = acc[i];
    }
}

// ---------------------------------------------------------------- conv weight gradient: split-K GEMM into slabs
// dW[co][tap * CI + ci] = sum_m dy[m][co] * x[n, y + ty - PAD, x + tx - PAD, ci] over the KCH rows m of slab blockIdx.y.
// Tile CO x BNW (BNW = 64 at CO = 64, 32 at CO = 128), one 32 x 32 accumulator per wave.  slab [S][CO][KS*KS*CI].
template <int KS, int CI, int CO, int H, int KCH>
__global__ __launch_bounds__(256) void k_twgrad(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ slab) {
    constexpr int WR = CO / 32, WC = 4 / WR, BNW = 32 * WC, BK = 32, LDA = CO + 4, LDB = BNW + 4, PAD = KS / 2, NW = KS * KS * CI;
    constexpr int AV = CO / 32, BV = BNW / 32;                 // vec4 loads per thread and K tile
    static_assert((CO == 64 || CO == 128) && CI % 4 == 0 && KCH % BK == 0, "tile geometry");
    __shared__ __attribute__((aligned(16))) float sA[BK][LDA];
    __shared__ __attribute__((aligned(16))) float sB[BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wr = wave % WR, wc = wave / WR;
    const int n0 = blockIdx.x * BNW;
    const int64_t kbase = (int64_t)blockIdx.y * KCH;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < KCH; k0 += BK) {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int v = tid + 256 * i, kk = v / (CO / 4), c4 = (v % (CO / 4)) * 4;
            const f32x4 a = *reinterpret_cast<const f32x4*>(dy + (size_t)(kbase + k0 + kk) * CO + c4);
            *reinterpret_cast<f32x4*>(&sA[kk][c4]) = a;
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int v = tid + 256 * i, kk = v / (BNW / 4), c4 = (v % (BNW / 4)) * 4;
            const int col = n0 + c4;
            const int64_t m = kbase + k0 + kk;
            const int xx = (int)(m % H), yy = (int)((m / H) % H);
            const int64_t n = m / (H * H);
            f32x4 b = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col < NW) {
                const int tap = col / CI, ci = col % CI;
                const int iy = yy + tap / KS - PAD, ix = xx + tap % KS - PAD;
                if (iy >= 0 && iy < H && ix >= 0 && ix < H)
                    b = *reinterpret_cast<const f32x4*>(x + (((size_t)n * H + iy) * H + ix) * CI + ci);
            }
            *reinterpret_cast<f32x4*>(&sB[kk][c4]) = b;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[2 * s + lh][wr * 32 + li], sB[2 * s + lh][wc * 32 + li], acc, 0, 0, 0);
        __syncthreads();
    }
    float* o = slab + (size_t)blockIdx.y * CO * NW;
    const int col = n0 + wc * 32 + li;
    if (col < NW) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            o[(size_t)row * NW + col] = acc[r];
        }
    }
}
// ordered slab sum; packed [co][t * CI + ci] -> torch (co, ci, t)
__global__ void k_wgrad_sum(const float* __restrict__ slab, int S, int CO, int CI, int T, float* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, n = (int64_t)CO * CI * T;
    if (i >= n) return;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += slab[(size_t)s * n + i];
    const int ci = (int)(i % CI), t = (int)((i / CI) % T), co = (int)(i / ((int64_t)CI * T));
    g[((int64_t)co * CI + ci) * T + t] = a;
}
// out[i] = sum_s slab[s][i]
__global__ void k_slab_sum(const float* __restrict__ slab, int S, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += slab[(size_t)s * n + i];
    out[i] = a;
}

// ---------------------------------------------------------------- BatchNorm batch statistics, per half
// y [rows][C]; block b covers rows [b * R, (b + 1) * R), all inside one half of Mh rows.  MODE 0: sum y; MODE 1: sum (y - mean)^2.
template <int MODE>
__global__ __launch_bounds__(256) void k_colred(const float* __restrict__ y, int C, int R, int64_t Mh, const float* __restrict__ mean,
                                                float* __restrict__ partial) {
    __shared__ float sred[256];
    const int tid = threadIdx.x, c = tid % C, g = tid / C, G = 256 / C;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int half = (int)(r0 / Mh);
    const float mu = MODE ? mean[half * C + c] : 0.f;
    float acc = 0.f;
    for (int r = g; r < R; r += G) {
        const float v = y[(size_t)(r0 + r) * C + c];
        if (MODE) { const float d = v - mu; acc = fmaf(d, d, acc); } else acc += v;
    }
    sred[tid] = acc;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < G; ++k) acc += sred[k * C + c];
        partial[(size_t)blockIdx.x * C + c] = acc;
    }
}
// phase 0: mean[h][c]; phase 1: invstd[h][c] and the running tensors (x1's half, then x2's).  One thread per channel.
__global__ void k_bnfin(const float* __restrict__ partial, int nper, int C, int64_t Mh, int phase, float eps,
                        const float* __restrict__ cbias, float* __restrict__ mean, float* __restrict__ invstd,
                        float* __restrict__ rmean, float* __restrict__ rvar) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    for (int h = 0; h < 2; ++h) {
        float s = 0.f;
        for (int b = 0; b < nper; ++b) s += partial[((size_t)h * nper + b) * C + c];
        if (phase == 0) {
            mean[h * C + c] = s / (float)Mh;
        } else {
            const float var = s / (float)Mh;
            invstd[h * C + c] = 1.0f / sqrtf(var + eps);
            rmean[c] = (1.0f - BN_MOMENTUM) * rmean[c] + BN_MOMENTUM * (mean[h * C + c] + cbias[c]);
            rvar[c] = (1.0f - BN_MOMENTUM) * rvar[c] + BN_MOMENTUM * (s / (float)(Mh - 1));
        }
    }
}
// BatchNorm + ReLU + 2x2 max: thread = pooled element (q, c).  pooled / route: NHWC (q * C + c), or torch's NCHW when NCHW.
template <bool NCHW>
__global__ void k_bnpool(const float* __restrict__ y, int C, int H, int64_t Qh /* pooled positions per half */, int64_t total,
                         const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                         const float* __restrict__ beta, float* __restrict__ pooled, uint8_t* __restrict__ route) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), HP = H / 2;
    const int64_t q = i / C;
    const int pw = (int)(q % HP), ph = (int)((q / HP) % HP);
    const int64_t n = q / (HP * HP);
    const int half = (int)(q / Qh);
    const float mu = mean[half * C + c], is = invstd[half * C + c], ga = gamma[c], be = beta[c];
    float best = 0.f; int idx = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = y[((size_t)(n * H + 2 * ph + (e >> 1)) * H + 2 * pw + (e & 1)) * C + c];
        const float z = (v - mu) * is * ga + be;
        if (e == 0 || z > best) { best = z; idx = e; }
    }
    const int64_t o = NCHW ? ((n * C + c) * HP + ph) * HP + pw : i;
    pooled[o] = fmaxf(best, 0.f);
    route[o] = best > 0.f ? (uint8_t)idx : (uint8_t)4;
}
// backward sums: block = CH pooled positions of one half; partial [blk][2][C] = sum dz, sum dz * xhat
template <bool NCHW>
__global__ __launch_bounds__(256) void k_bnbwd_red(const float* __restrict__ dpool, const uint8_t* __restrict__ route,
                                                   const float* __restrict__ y, int C, int H, int CH, int64_t Qh,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                   float* __restrict__ partial) {
    __shared__ float s1[256], s2[256];
    const int tid = threadIdx.x, c = tid % C, g = tid / C, G = 256 / C, HP = H / 2;
    const int64_t q0 = (int64_t)blockIdx.x * CH;
    const int half = (int)(q0 / Qh);
    const float mu = mean[half * C + c], is = invstd[half * C + c];
    float a1 = 0.f, a2 = 0.f;
    for (int k = g; k < CH; k += G) {
        const int64_t q = q0 + k;
        const int pw = (int)(q % HP), ph = (int)((q / HP) % HP);
        const int64_t n = q / (HP * HP);
        const int64_t o = NCHW ? ((n * C + c) * HP + ph) * HP + pw : q * C + c;
        const int r = route[o];
        if (r < 4) {
            const float d = dpool[o];
            const float v = y[((size_t)(n * H + 2 * ph + (r >> 1)) * H + 2 * pw + (r & 1)) * C + c];
            a1 += d;
            a2 = fmaf(d, (v - mu) * is, a2);
        }
    }
    s1[tid] = a1; s2[tid] = a2;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < G; ++k) { a1 += s1[k * C + c]; a2 += s2[k * C + c]; }
        partial[((size_t)blockIdx.x * 2) * C + c] = a1;
        partial[((size_t)blockIdx.x * 2 + 1) * C + c] = a2;
    }
}
// sums [h][2][C]; dgamma = sum over both halves of sum dz * xhat, dbeta of sum dz
__global__ void k_bnbwd_fin(const float* __restrict__ partial, int nper, int C, float* __restrict__ sums,
                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float t1[2], t2[2];
    for (int h = 0; h < 2; ++h) {
        float a1 = 0.f, a2 = 0.f;
        for (int b = 0; b < nper; ++b) {
            a1 += partial[(((size_t)h * nper + b) * 2) * C + c];
            a2 += partial[(((size_t)h * nper + b) * 2 + 1) * C + c];
        }
        sums[(h * 2) * C + c] = a1; sums[(h * 2 + 1) * C + c] = a2;
        t1[h] = a1; t2[h] = a2;
    }
    dbeta[c] = t1[0] + t1[1];
    dgamma[c] = t2[0] + t2[1];
}
// dy = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)); thread = pooled element, writes its four pixels
template <bool NCHW>
__global__ void k_bnbwd_apply(const float* __restrict__ dpool, const uint8_t* __restrict__ route, const float* __restrict__ y,
                              int C, int H, int64_t Qh, int64_t total, const float* __restrict__ mean,
                              const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ sums,
                              float* __restrict__ dy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), HP = H / 2;
    const int64_t q = i / C;
    const int pw = (int)(q % HP), ph = (int)((q / HP) % HP);
    const int64_t n = q / (HP * HP);
    const int half = (int)(q / Qh);
    const float mu = mean[half * C + c], is = invstd[half * C + c];
    const float inv_m = 1.0f / (float)(Qh * 4);
    const float m1 = sums[(half * 2) * C + c] * inv_m, m2 = sums[(half * 2 + 1) * C + c] * inv_m, gi = gamma[c] * is;
    const int64_t o = NCHW ? ((n * C + c) * HP + ph) * HP + pw : i;
    const int r = route[o];
    const float d = dpool[o];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const size_t a = ((size_t)(n * H + 2 * ph + (e >> 1)) * H + 2 * pw + (e & 1)) * C + c;
        const float xh = (y[a] - mu) * is;
        dy[a] = gi * ((r == e ? d : 0.f) - m1 - xh * m2);
    }
}

// ---------------------------------------------------------------- tail: fc1 finish + dropout, fc2, L2 normalise (one block per row)
struct Rng { unsigned long long seed, ctr; };
__global__ __launch_bounds__(256) void k_ttail(const float* __restrict__ part, int M, int nsplit, const float* __restrict__ b1,
                                               const float* __restrict__ w2 /* (E, 512) */, const float* __restrict__ b2, int E,
                                               const float* __restrict__ keep_in, Rng rng, float* __restrict__ hdrop,
                                               float* __restrict__ hmul, uint8_t* __restrict__ relu1, uint8_t* __restrict__ keep1,
                                               float* __restrict__ eraw, float* __restrict__ nrm_out, float* __restrict__ emb) {
    extern __shared__ float se[];                      // E embedding entries
    __shared__ float sh1[VFC1_N];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int half = row >= nsplit;
    for (int j = tid; j < VFC1_N; j += 256) {
        const float a = fc1_finish(part, M, row, j, b1);
        const size_t o = (size_t)row * VFC1_N + j;
        const bool keep = keep_in ? keep_in[o] != 0.f
                                  : drawn_keep(rng.seed, rng.ctr, (uint64_t)(row - half * nsplit) * VFC1_N + j, half ? SID_FC2 : SID_FC1, 1.0f - P_FC);
        const float mul = keep ? 1.0f / (1.0f - P_FC) : 0.f;
        const float h = a * mul;
        sh1[j] = h;
        hdrop[o] = h;
        hmul[o] = a > 0.f ? mul : 0.f;
        relu1[o] = a > 0.f;
        keep1[o] = keep;
    }
    const float nrm = fc2_norm(sh1, w2, b2, E, se);
    if (tid == 0) nrm_out[row] = nrm;
    for (int i = tid; i < E; i += 256) {
        eraw[(size_t)row * E + i] = se[i];
        emb[(size_t)row * E + i] = se[i] / nrm;
    }
}

// ---------------------------------------------------------------- pair head: forward, losses, backward to d(e1) (64 threads per pair)
// pm [B][4] = bce, contrastive term, correct, d(logit)
__global__ __launch_bounds__(64) void k_thead(const float* __restrict__ emb, int B, int E, const float* __restrict__ w0,
                                              const float* __restrict__ b0, const float* __restrict__ w3, const float* __restrict__ b3,
                                              const float* __restrict__ labels, const float* __restrict__ keep_in, Rng rng,
                                              int use_c, float* __restrict__ absd, float* __restrict__ hd_out,
                                              float* __restrict__ dhid_out, float* __restrict__ de, float* __restrict__ sim,
                                              float* __restrict__ dist, float* __restrict__ pm, uint8_t* __restrict__ relu_c,
                                              uint8_t* __restrict__ keep_c) {
    extern __shared__ float sd[];                      // E signed differences
    __shared__ float sdh[VHID];
    const int p = blockIdx.x, j = threadIdx.x;
    const float* e1 = emb + (size_t)p * E;
    const float* e2 = emb + (size_t)(B + p) * E;
    float dq = 0.f;
    for (int k = j; k < E; k += VHID) {
        const float d = e1[k] - e2[k];
        sd[k] = d;
        absd[(size_t)p * E + k] = fabsf(d);
        const float t = d + 1e-6f;                     // F.pairwise_distance adds its eps to the difference
        dq = fmaf(t, t, dq);
    }
    __syncthreads();
    const float D = sqrtf(wave_sum(dq));
    const float* wr = w0 + (size_t)j * E;
    float a = 0.f;
    for (int k = 0; k < E; ++k) a = fmaf(fabsf(sd[k]), wr[k], a);
    a = fmaxf(a + b0[j], 0.f);
    const size_t o = (size_t)p * VHID + j;
    const bool keep = keep_in ? keep_in[o] != 0.f : drawn_keep(rng.seed, rng.ctr, (uint64_t)o, SID_CLS, 1.0f - P_CLS);
    const float mul = keep ? 1.0f / (1.0f - P_CLS) : 0.f;
    const float hd = a * mul;
    relu_c[o] = a > 0.f;
    keep_c[o] = keep;
    hd_out[o] = hd;
    const float logit = wave_sum(hd * w3[j]) + b3[0];
    const float s = 1.0f / (1.0f + expf(-logit));
    const float yv = labels[p];
    // BCELoss with torch's -100 clamp of the logs; backward (p - y) / max((1 - p) p, 1e-12), mean over the batch
    const float bce = -(yv * fmaxf(logf(s), -100.f) + (1.0f - yv) * fmaxf(logf(1.0f - s), -100.f));
    const float dsim = (s - yv) / fmaxf((1.0f - s) * s, 1e-12f) / (float)B;
    const float dlogit = dsim * ((1.0f - s) * s);
    const float gap = fmaxf(2.0f - D, 0.f);
    const float cterm = yv * D * D + (1.0f - yv) * gap * gap;
    const float dh = a > 0.f ? dlogit * w3[j] * mul : 0.f;
    dhid_out[o] = dh;
    sdh[j] = dh;
    if (j == 0) {
        sim[p] = s;
        dist[p] = D;
        pm[p * 4 + 0] = bce;
        pm[p * 4 + 1] = cterm;
        pm[p * 4 + 2] = ((s > 0.5f ? 1.0f : 0.0f) == yv) ? 1.0f : 0.0f;
        pm[p * 4 + 3] = dlogit;
    }
    __syncthreads();
    // loss = bce + 0.5 * mean(cterm): d/dD = 0.5 / B * (2 y D - 2 (1 - y) clamp(2 - D, 0))
    const float gD = use_c ? 0.5f / (float)B * (2.0f * yv * D - 2.0f * (1.0f - yv) * gap) : 0.f;
    for (int k = j; k < E; k += VHID) {
        float da = 0.f;
        for (int i = 0; i < VHID; ++i) da = fmaf(sdh[i], w0[(size_t)i * E + k], da);
        const float d = sd[k];
        float g = d > 0.f ? da : (d < 0.f ? -da : 0.f);                 // |.|' = sign, 0 at 0
        if (use_c && D > 0.f) g += gD * ((d + 1e-6f) / D);
        de[(size_t)p * E + k] = g;
    }
}
// batch sums of the head: classifier.0.weight / .bias, classifier.3.weight / .bias gradients and the metrics; one thread
// per output, pairs in order
__global__ void k_thead_sum(const float* __restrict__ dhid, const float* __restrict__ absd, const float* __restrict__ hd,
                            const float* __restrict__ pm, int B, int E, int use_c, float* __restrict__ gw0, float* __restrict__ gb0,
                            float* __restrict__ gw3, float* __restrict__ gb3, float* __restrict__ metrics) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, nw0 = VHID * E;
    if (i < nw0) {
        const int jj = i / E, k = i % E;
        float a = 0.f;
        for (int p = 0; p < B; ++p) a = fmaf(dhid[(size_t)p * VHID + jj], absd[(size_t)p * E + k], a);
        gw0[i] = a;
    } else if (i < nw0 + VHID) {
        const int jj = i - nw0;
        float a = 0.f, b = 0.f;
        for (int p = 0; p < B; ++p) { a += dhid[(size_t)p * VHID + jj]; b = fmaf(pm[p * 4 + 3], hd[(size_t)p * VHID + jj], b); }
        gb0[jj] = a;
        gw3[jj] = b;
    } else if (i == nw0 + VHID) {
        float a = 0.f, bce = 0.f, ct = 0.f, nc = 0.f;
        for (int p = 0; p < B; ++p) { a += pm[p * 4 + 3]; bce += pm[p * 4 + 0]; ct += pm[p * 4 + 1]; nc += pm[p * 4 + 2]; }
        gb3[0] = a;
        if (metrics) {
            bce /= (float)B;
            ct = use_c ? ct / (float)B : 0.f;
            metrics[0] = bce + 0.5f * ct; metrics[1] = bce; metrics[2] = ct; metrics[3] = nc;
        }
    }
}

// ---------------------------------------------------------------- per row: normalise / fc2 / dropout / ReLU backward
__global__ __launch_bounds__(256) void k_tembbwd(const float* __restrict__ de, int B, int E, const float* __restrict__ eraw,
                                                 const float* __restrict__ nrm_in, const float* __restrict__ emb,
                                                 const float* __restrict__ w2, const float* __restrict__ hmul,
                                                 float* __restrict__ deraw, float* __restrict__ dH) {
    extern __shared__ float sg[];                      // E raw-embedding gradients
    __shared__ float sred[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = row < B ? row : row - B;
    const float sign = row < B ? 1.0f : -1.0f;
    const float nrm = nrm_in[row];
    float dot = 0.f;
    for (int k = tid; k < E; k += 256) dot = fmaf(sign * de[(size_t)p * E + k], emb[(size_t)row * E + k], dot);
    dot = wave_sum(dot);
    if (lane == 0) sred[wave] = dot;
    __syncthreads();
    dot = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    for (int k = tid; k < E; k += 256) {
        // x / max(||x||, eps): above eps d = (g - e (g . e)) / ||x||; clamped (||x|| <= eps) it is g / eps
        const float g = sign * de[(size_t)p * E + k];
        const float v = nrm > 1e-12f ? (g - emb[(size_t)row * E + k] * dot) / nrm : g / nrm;
        sg[k] = v;
        deraw[(size_t)row * E + k] = v;
    }
    __syncthreads();
    for (int j = tid; j < VFC1_N; j += 256) {
        float a = 0.f;
        for (int o = 0; o < E; ++o) a = fmaf(sg[o], w2[(size_t)o * VFC1_N + j], a);
        dH[(size_t)row * VFC1_N + j] = a * hmul[(size_t)row * VFC1_N + j];
    }
}
// fc2.weight (E, 512), fc2.bias (E), fc1.bias (512) gradients: one thread per output, rows in order
__global__ void k_tfc2_sum(const float* __restrict__ deraw, const float* __restrict__ hdrop, const float* __restrict__ dH, int M,
                           int E, float* __restrict__ gw2, float* __restrict__ gb2, float* __restrict__ gb1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nw = (int64_t)E * VFC1_N;
    if (i < nw) {
        const int o = (int)(i / VFC1_N), j = (int)(i % VFC1_N);
        float a = 0.f;
        for (int r = 0; r < M; ++r) a = fmaf(deraw[(size_t)r * E + o], hdrop[(size_t)r * VFC1_N + j], a);
        gw2[i] = a;
    } else if (i < nw + E) {
        const int o = (int)(i - nw);
        float a = 0.f;
        for (int r = 0; r < M; ++r) a += deraw[(size_t)r * E + o];
        gb2[o] = a;
    } else if (i < nw + E + VFC1_N) {
        const int j = (int)(i - nw - E);
        float a = 0.f;
        for (int r = 0; r < M; ++r) a += dH[(size_t)r * VFC1_N + j];
        gb1[j] = a;
    }
}

}  // namespace

// parameter tensors in named_parameters() order
enum { P_C1W = 0, P_C1B, P_G1, P_B1, P_C2W, P_C2B, P_G2, P_B2, P_C3W, P_C3B, P_G3, P_B3, P_F1W, P_F1B, P_F2W, P_F2B, P_K0W, P_K0B, P_K3W, P_K3B };

struct siggan_verifier_trainer {
    int device, E, Bmax;
    bool bound;
    int last_b;                          // pairs of the last _grads call (0: none yet)
    int64_t off[SIGGAN_VT_PARAM_TENSORS + 1];
    siggan_verifier_train_storage st;
    unsigned long long seed, rng_ctr;
    double adam_t;
    char* ws;
    DevState* dst; float* steps;
    float *wp2, *wf2, *wp3, *wf3;
    float *y1, *y2, *y3, *pool1, *pool2, *pool3, *dy1, *dy2, *dy3, *dp1, *dp2, *dp3;
    uint8_t *r1, *r2, *r3, *relu1, *keep1, *reluc, *keepc;
    float *bnpart, *mean, *invstd, *bsums;     // mean / invstd: [layer][2][128]; bsums [layer][2][2][128]
    float *part, *hdrop, *hmul, *eraw, *nrm, *emb, *deraw, *dH;
    float *absd, *hd, *dhid, *de, *sim, *dist, *pm;
    float* slab;
};

extern "C" int siggan_verifier_trainer_create(int32_t device, int32_t E, int32_t max_pairs, siggan_verifier_trainer** out) {
    if (!out) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_create: null argument");
    *out = nullptr;
    if (E < 1 || E > SIGGAN_VERIFIER_MAX_EMBEDDING)
        return FAIL(SIGGAN_E_ARG, "embedding_dim %d outside [1, %d]", E, SIGGAN_VERIFIER_MAX_EMBEDDING);
    if (max_pairs < 1 || max_pairs > 1024) return FAIL(SIGGAN_E_ARG, "max_pairs %d outside [1, 1024]", max_pairs);
    DevGuard dg(device); HIPCHK(dg.err);
    siggan_verifier_trainer* t = new (std::nothrow) siggan_verifier_trainer();
    if (!t) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    t->device = device; t->E = E; t->Bmax = max_pairs; t->bound = false; t->last_b = 0; t->ws = nullptr;
    t->seed = 0; t->rng_ctr = 0; t->adam_t = 0.0;
    const int64_t cnt[SIGGAN_VT_PARAM_TENSORS] = {800, 32, 32, 32, 51200, 64, 64, 64, 73728, 128, 128, 128, (int64_t)VFC1_N * VFC1_K, VFC1_N,
                                                  (int64_t)E * VFC1_N, E, (int64_t)VHID * E, VHID, VHID, 1};
    t->off[0] = 0;
    for (int i = 0; i < SIGGAN_VT_PARAM_TENSORS; ++i) t->off[i + 1] = t->off[i] + cnt[i];
    const int64_t B = max_pairs, N = 2 * B;
    size_t off = 0; char* base = nullptr;
    auto carve = [&](void* pp, int64_t bytes) { if (base) *(void**)pp = (void*)(base + off); off += ((size_t)bytes + 255) & ~(size_t)255; };
    auto cf = [&](float** p, int64_t n) { carve(p, n * 4); };
    auto cb = [&](uint8_t** p, int64_t n) { carve(p, n); };
    // slabs: conv2 N x 64 x 800, conv3 N x 128 x 576, conv1 4N x 800
    const int64_t nslab = N * 128 * 576;
    // BatchNorm partial rows: forward 2 * 4B blocks of <= 128 channels, backward 2B blocks x 2 x 128
    const int64_t nbnpart = N * 4 * 128;
    for (int pass = 0; pass < 2; ++pass) {
        off = 0;
        carve(&t->dst, sizeof(DevState)); cf(&t->steps, 32);
        cf(&t->wp2, 51200); cf(&t->wf2, 51200); cf(&t->wp3, 73728); cf(&t->wf3, 73728);
        cf(&t->y1, N * 4096 * 32); cf(&t->y2, N * 1024 * 64); cf(&t->y3, N * 256 * 128);
        cf(&t->dy1, N * 4096 * 32); cf(&t->dy2, N * 1024 * 64); cf(&t->dy3, N * 256 * 128);
        cf(&t->pool1, N * 1024 * 32); cf(&t->pool2, N * 256 * 64); cf(&t->pool3, N * VFC1_K);
        cf(&t->dp1, N * 1024 * 32); cf(&t->dp2, N * 256 * 64); cf(&t->dp3, N * VFC1_K);
        cb(&t->r1, N * 1024 * 32); cb(&t->r2, N * 256 * 64); cb(&t->r3, N * VFC1_K);
        cb(&t->relu1, N * VFC1_N); cb(&t->keep1, N * VFC1_N); cb(&t->reluc, B * VHID); cb(&t->keepc, B * VHID);
        cf(&t->bnpart, nbnpart); cf(&t->mean, 3 * 2 * 128); cf(&t->invstd, 3 * 2 * 128); cf(&t->bsums, 3 * 4 * 128);
        cf(&t->part, N * VFC1_SPLIT * VFC1_N); cf(&t->hdrop, N * VFC1_N); cf(&t->hmul, N * VFC1_N);
        cf(&t->eraw, N * E); cf(&t->nrm, N); cf(&t->emb, N * E); cf(&t->deraw, N * E); cf(&t->dH, N * VFC1_N);
        cf(&t->absd, B * E); cf(&t->hd, B * VHID); cf(&t->dhid, B * VHID); cf(&t->de, B * E); cf(&t->sim, B); cf(&t->dist, B);
        cf(&t->pm, B * 4);
        cf(&t->slab, nslab);
        if (pass == 0) {
            hipError_t e = hipMalloc((void**)&base, off);
            if (e != hipSuccess) { delete t; return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", off, hipGetErrorString(e)); }
            t->ws = base;
        }
    }
    hipError_t e = hipMemset(t->dst, 0, sizeof(DevState));
    if (e == hipSuccess) e = hipMemset(t->steps, 0, 32 * 4);
    if (e != hipSuccess) { (void)hipFree(t->ws); delete t; return FAIL(SIGGAN_E_HIP, "hipMemset -> %s", hipGetErrorString(e)); }
    *out = t;
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_trainer_destroy(siggan_verifier_trainer* t) {
    if (!t) return SIGGAN_OK;
    DevGuard dg(t->device);
    (void)hipDeviceSynchronize();
    if (t->ws) (void)hipFree(t->ws);
    delete t;
    return SIGGAN_OK;
}

extern "C" int64_t siggan_verifier_trainer_param_count(const siggan_verifier_trainer* t) {
    return t ? t->off[SIGGAN_VT_PARAM_TENSORS] : 0;
}

extern "C" int siggan_verifier_trainer_param_span(const siggan_verifier_trainer* t, int32_t index, int64_t* offset, int64_t* count) {
    if (!t || !offset || !count) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_param_span: null argument");
    if (index < 0 || index >= SIGGAN_VT_PARAM_TENSORS)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_param_span: index %d outside [0, %d)", index, SIGGAN_VT_PARAM_TENSORS);
    *offset = t->off[index];
    *count = t->off[index + 1] - t->off[index];
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_trainer_bind(siggan_verifier_trainer* t, const siggan_verifier_train_storage* s, int64_t adam_step) {
    if (!t || !s) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_bind: null argument");
    const float* const* p = reinterpret_cast<const float* const*>(s);
    for (int i = 0; i < 10; ++i)
        if (!p[i]) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_bind: storage pointer %d is null", i);
    if (!(s->bn_eps > 0.f)) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_bind: bn_eps must be positive");
    if (adam_step < 0) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_bind: adam_step %lld < 0", (long long)adam_step);
    if (((uintptr_t)s->params | (uintptr_t)s->grads | (uintptr_t)s->exp_avg | (uintptr_t)s->exp_avg_sq) & 15)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_bind: the arenas must be 16-byte aligned");
    t->st = *s;
    t->adam_t = (double)adam_step;
    t->bound = true;
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_trainer_seed(siggan_verifier_trainer* t, uint64_t seed, uint64_t offset) {
    if (!t) return FAIL(SIGGAN_E_ARG, "siggan_verifier_trainer_seed: null context");
    t->seed = seed; t->rng_ctr = offset;
    return SIGGAN_OK;
}

static int tcheck(const siggan_verifier_trainer* t, const char* fn) {
    if (!t) return FAIL(SIGGAN_E_ARG, "%s: null context", fn);
    if (!t->bound) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_trainer_bind has not been called", fn);
    return SIGGAN_OK;
}

// one conv layer's statistics + pooling: y (N, H, H, C) -> pooled, route
template <bool NCHW>
static void bn_forward(siggan_verifier_trainer* t, int layer, const float* y, int C, int H, int R, int B, const float* cbias,
                       const float* gamma, const float* beta, float* rmean, float* rvar, float* pooled, uint8_t* route, hipStream_t s) {
    const int64_t Mh = (int64_t)B * H * H;
    const int nper = (int)(Mh / R);
    float* mean = t->mean + layer * 256;
    float* invstd = t->invstd + layer * 256;
    hipLaunchKernelGGL(k_colred<0>, dim3(2 * nper), dim3(256), 0, s, y, C, R, Mh, (const float*)nullptr, t->bnpart);
    hipLaunchKernelGGL(k_bnfin, dim3(1), dim3(128), 0, s, t->bnpart, nper, C, Mh, 0, t->st.bn_eps, cbias, mean, invstd, rmean, rvar);
    hipLaunchKernelGGL(k_colred<1>, dim3(2 * nper), dim3(256), 0, s, y, C, R, Mh, (const float*)mean, t->bnpart);
    hipLaunchKernelGGL(k_bnfin, dim3(1), dim3(128), 0, s, t->bnpart, nper, C, Mh, 1, t->st.bn_eps, cbias, mean, invstd, rmean, rvar);
    const int64_t Qh = Mh / 4, total = 2 * Qh * C;
    hipLaunchKernelGGL(k_bnpool<NCHW>, dim3(blocks(total)), dim3(256), 0, s, y, C, H, Qh, total, (const float*)mean, (const float*)invstd,
                       gamma, beta, pooled, route);
}
// d(pooled) -> dy, dgamma, dbeta
template <bool NCHW>
static void bn_backward(siggan_verifier_trainer* t, int layer, const float* dpool, const uint8_t* route, const float* y, int C, int H,
                        int CH, int B, const float* gamma, float* dgamma, float* dbeta, float* dy, hipStream_t s) {
    const int64_t Qh = (int64_t)B * (H / 2) * (H / 2);
    const int nper = (int)(Qh / CH);
    const float* mean = t->mean + layer * 256;
    const float* invstd = t->invstd + layer * 256;
    float* sums = t->bsums + layer * 512;
    hipLaunchKernelGGL(k_bnbwd_red<NCHW>, dim3(2 * nper), dim3(256), 0, s, dpool, route, y, C, H, CH, Qh, mean, invstd, t->bnpart);
    hipLaunchKernelGGL(k_bnbwd_fin, dim3(1), dim3(128), 0, s, (const float*)t->bnpart, nper, C, sums, dgamma, dbeta);
    const int64_t total = 2 * Qh * C;
    hipLaunchKernelGGL(k_bnbwd_apply<NCHW>, dim3(blocks(total)), dim3(256), 0, s, dpool, route, y, C, H, Qh, total, mean, invstd, gamma,
                       (const float*)sums, dy);
}

static int train_grads(siggan_verifier_trainer* t, const void* x1, const void* x2, int fmt, const float* labels, int B,
                       const float* fc_keep, const float* cls_keep, int use_c, float* metrics, hipStream_t s) {
    const int N = 2 * B, E = t->E;
    const float* P = t->st.params;
    float* G = t->st.grads;
    auto p = [&](int i) { return P + t->off[i]; };
    auto g = [&](int i) { return G + t->off[i]; };
    const Rng rng{t->seed, t->rng_ctr};
    t->rng_ctr += 1;
    // ---- packs
    hipLaunchKernelGGL(k_tpack, dim3(blocks(51200)), dim3(256), 0, s, p(P_C2W), t->wp2, t->wf2, 64, 32, 25);
    hipLaunchKernelGGL(k_tpack, dim3(blocks(73728)), dim3(256), 0, s, p(P_C3W), t->wp3, t->wf3, 128, 64, 9);
    // ---- forward
    if (fmt == SIGGAN_VFMT_U8) hipLaunchKernelGGL(k_tconv1<true>, dim3(N * 64), dim3(256), 0, s, x1, x2, B, p(P_C1W), t->y1);
    else hipLaunchKernelGGL(k_tconv1<false>, dim3(N * 64), dim3(256), 0, s, x1, x2, B, p(P_C1W), t->y1);
    bn_forward<false>(t, 0, t->y1, 32, 64, 1024, B, p(P_C1B), p(P_G1), p(P_B1), t->st.bn1_running_mean, t->st.bn1_running_var, t->pool1, t->r1, s);
    hipLaunchKernelGGL((k_tconv<5, 32, 64, 32, 64>), dim3(N * 1024 / 128, 1), dim3(256), 0, s, (const float*)t->pool1, (const float*)t->wp2, t->y2);
    bn_forward<false>(t, 1, t->y2, 64, 32, 256, B, p(P_C2B), p(P_G2), p(P_B2), t->st.bn2_running_mean, t->st.bn2_running_var, t->pool2, t->r2, s);
    hipLaunchKernelGGL((k_tconv<3, 64, 128, 16, 64>), dim3(N * 256 / 128, 2), dim3(256), 0, s, (const float*)t->pool2, (const float*)t->wp3, t->y3);
    bn_forward<true>(t, 2, t->y3, 128, 16, 256, B, p(P_C3B), p(P_G3), p(P_B3), t->st.bn3_running_mean, t->st.bn3_running_var, t->pool3, t->r3, s);
    hipLaunchKernelGGL((k_tgemm<true, true>), dim3(VFC1_N / 64, (N + 63) / 64, VFC1_SPLIT), dim3(256), 0, s, (const float*)t->pool3, p(P_F1W), t->part,
                       N, VFC1_N, VFC1_K, VFC1_KS, VFC1_K, VFC1_K, VFC1_N);
    hipLaunchKernelGGL(k_ttail, dim3(N), dim3(256), (size_t)E * 4, s, (const float*)t->part, N, B, p(P_F1B), p(P_F2W), p(P_F2B), E, fc_keep, rng,
                       t->hdrop, t->hmul, t->relu1, t->keep1, t->eraw, t->nrm, t->emb);
    hipLaunchKernelGGL(k_thead, dim3(B), dim3(VHID), (size_t)E * 4, s, (const float*)t->emb, B, E, p(P_K0W), p(P_K0B), p(P_K3W), p(P_K3B), labels,
                       cls_keep, rng, use_c, t->absd, t->hd, t->dhid, t->de, t->sim, t->dist, t->pm, t->reluc, t->keepc);
    // ---- backward: head, embedding, fc
    hipLaunchKernelGGL(k_thead_sum, dim3(blocks(VHID * E + VHID + 1)), dim3(256), 0, s, (const float*)t->dhid, (const float*)t->absd,
                       (const float*)t->hd, (const float*)t->pm, B, E, use_c, g(P_K0W), g(P_K0B), g(P_K3W), g(P_K3B), metrics);
    hipLaunchKernelGGL(k_tembbwd, dim3(N), dim3(256), (size_t)E * 4, s, (const float*)t->de, B, E, (const float*)t->eraw, (const float*)t->nrm,
                       (const float*)t->emb, p(P_F2W), (const float*)t->hmul, t->deraw, t->dH);
    hipLaunchKernelGGL(k_tfc2_sum, dim3(blocks((int64_t)E * VFC1_N + E + VFC1_N)), dim3(256), 0, s, (const float*)t->deraw, (const float*)t->hdrop,
                       (const float*)t->dH, N, E, g(P_F2W), g(P_F2B), g(P_F1B));
    // d(pool3) (N, 8192) = dH (N, 512) . W (512, 8192);  dW (512, 8192) = dH^T . pool3
    hipLaunchKernelGGL((k_tgemm<true, false>), dim3(VFC1_K / 64, (N + 63) / 64, 1), dim3(256), 0, s, (const float*)t->dH, p(P_F1W), t->dp3,
                       N, VFC1_K, VFC1_N, VFC1_N, VFC1_N, VFC1_K, VFC1_K);
    hipLaunchKernelGGL((k_tgemm<false, false>), dim3(VFC1_K / 64, VFC1_N / 64, 1), dim3(256), 0, s, (const float*)t->dH, (const float*)t->pool3, g(P_F1W),
                       VFC1_N, VFC1_K, N, ((N + 31) / 32) * 32, VFC1_N, VFC1_K, VFC1_K);
    // ---- conv3
    bn_backward<true>(t, 2, t->dp3, t->r3, t->y3, 128, 16, 64, B, p(P_G3), g(P_G3), g(P_B3), t->dy3, s);
    hipLaunchKernelGGL((k_twgrad<3, 64, 128, 16, 256>), dim3(576 / 32, N), dim3(256), 0, s, (const float*)t->dy3, (const float*)t->pool2, t->slab);
    hipLaunchKernelGGL(k_wgrad_sum, dim3(blocks(73728)), dim3(256), 0, s, (const float*)t->slab, N, 128, 64, 9, g(P_C3W));
    hipLaunchKernelGGL((k_tconv<3, 128, 64, 16, 64>), dim3(N * 256 / 128, 1), dim3(256), 0, s, (const float*)t->dy3, (const float*)t->wf3, t->dp2);
    // ---- conv2
    bn_backward<false>(t, 1, t->dp2, t->r2, t->y2, 64, 32, 256, B, p(P_G2), g(P_G2), g(P_B2), t->dy2, s);
    hipLaunchKernelGGL((k_twgrad<5, 32, 64, 32, 1024>), dim3((800 + 63) / 64, N), dim3(256), 0, s, (const float*)t->dy2, (const float*)t->pool1, t->slab);
    hipLaunchKernelGGL(k_wgrad_sum, dim3(blocks(51200)), dim3(256), 0, s, (const float*)t->slab, N, 64, 32, 25, g(P_C2W));
    hipLaunchKernelGGL((k_tconv<5, 64, 32, 32, 32>), dim3(N * 1024 / 128, 1), dim3(256), 0, s, (const float*)t->dy2, (const float*)t->wf2, t->dp1);
    // ---- conv1
    bn_backward<false>(t, 0, t->dp1, t->r1, t->y1, 32, 64, 1024, B, p(P_G1), g(P_G1), g(P_B1), t->dy1, s);
    if (fmt == SIGGAN_VFMT_U8) hipLaunchKernelGGL(k_tconv1_wgrad<true>, dim3(N * 4), dim3(256), 0, s, x1, x2, B, (const float*)t->dy1, t->slab);
    else hipLaunchKernelGGL(k_tconv1_wgrad<false>, dim3(N * 4), dim3(256), 0, s, x1, x2, B, (const float*)t->dy1, t->slab);
    hipLaunchKernelGGL(k_slab_sum, dim3(blocks(800)), dim3(256), 0, s, (const float*)t->slab, N * 4, (int64_t)800, g(P_C1W));
    // conv biases in front of a train-mode BatchNorm: the gradient is exactly zero
    if (hipMemsetAsync(g(P_C1B), 0, 32 * 4, s) != hipSuccess || hipMemsetAsync(g(P_C2B), 0, 64 * 4, s) != hipSuccess ||
        hipMemsetAsync(g(P_C3B), 0, 128 * 4, s) != hipSuccess)
        return FAIL(SIGGAN_E_HIP, "siggan_verifier_train_grads: hipMemsetAsync failed");
    t->last_b = B;
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_train_grads: kernel launch failed");
}

static int grads_args(const siggan_verifier_trainer* t, const char* fn, const void* x1, const void* x2, int fmt, const float* labels, int B) {
    int rc = tcheck(t, fn); if (rc) return rc;
    if (!x1 || !x2 || !labels) return FAIL(SIGGAN_E_ARG, "%s: null tensor", fn);
    if (fmt != SIGGAN_VFMT_F32 && fmt != SIGGAN_VFMT_U8) return FAIL(SIGGAN_E_ARG, "%s: unknown fmt %d", fn, fmt);
    if (B < 1 || B > t->Bmax) return FAIL(SIGGAN_E_ARG, "%s: n_pairs %d outside [1, max_pairs=%d]", fn, B, t->Bmax);
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_train_grads(siggan_verifier_trainer* t, const void* x1, const void* x2, int32_t fmt, const float* labels,
                                           int32_t B, const float* fc_keep, const float* cls_keep, int32_t use_c, float* metrics,
                                           void* stream) {
    int rc = grads_args(t, "siggan_verifier_train_grads", x1, x2, fmt, labels, B); if (rc) return rc;
    DevGuard dg(t->device); HIPCHK(dg.err);
    return train_grads(t, x1, x2, fmt, labels, B, fc_keep, cls_keep, use_c ? 1 : 0, metrics, (hipStream_t)stream);
}

static int train_apply(siggan_verifier_trainer* t, double lr, double beta1, double beta2, double eps, hipStream_t s) {
    t->adam_t += 1.0;
    launch_adam_fused(t->st.params, t->st.grads, t->st.exp_avg, t->st.exp_avg_sq, t->off[SIGGAN_VT_PARAM_TENSORS], t->dst, t->steps,
                      SIGGAN_VT_PARAM_TENSORS, t->adam_t, lr, beta1, beta2, eps, 1.0f, 0.f, nullptr, nullptr, s);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_train_apply: kernel launch failed");
}
static int apply_args(const siggan_verifier_trainer* t, const char* fn, double lr, double beta1, double beta2, double eps) {
    int rc = tcheck(t, fn); if (rc) return rc;
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return FAIL(SIGGAN_E_ARG, "%s: invalid Adam hyper-parameters", fn);
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_train_apply(siggan_verifier_trainer* t, double lr, double beta1, double beta2, double eps, void* stream) {
    int rc = apply_args(t, "siggan_verifier_train_apply", lr, beta1, beta2, eps); if (rc) return rc;
    DevGuard dg(t->device); HIPCHK(dg.err);
    return train_apply(t, lr, beta1, beta2, eps, (hipStream_t)stream);
}

extern "C" int siggan_verifier_train_step(siggan_verifier_trainer* t, const void* x1, const void* x2, int32_t fmt, const float* labels,
                                          int32_t B, const float* fc_keep, const float* cls_keep, int32_t use_c, double lr,
                                          double beta1, double beta2, double eps, float* metrics, void* stream) {
    int rc = grads_args(t, "siggan_verifier_train_step", x1, x2, fmt, labels, B); if (rc) return rc;
    if ((rc = apply_args(t, "siggan_verifier_train_step", lr, beta1, beta2, eps))) return rc;
    DevGuard dg(t->device); HIPCHK(dg.err);
    if ((rc = train_grads(t, x1, x2, fmt, labels, B, fc_keep, cls_keep, use_c ? 1 : 0, metrics, (hipStream_t)stream))) return rc;
    return train_apply(t, lr, beta1, beta2, eps, (hipStream_t)stream);
}

extern "C" int siggan_verifier_train_debug(siggan_verifier_trainer* t, const char* name, void* out, int64_t n, void* stream) {
    int rc = tcheck(t, "siggan_verifier_train_debug"); if (rc) return rc;
    if (!name || !out) return FAIL(SIGGAN_E_ARG, "siggan_verifier_train_debug: null argument");
    if (t->last_b < 1) return FAIL(SIGGAN_E_ARG, "siggan_verifier_train_debug: no _grads call yet");
    const int64_t B = t->last_b, N = 2 * B, E = t->E;
    const void* src = nullptr; int64_t total = 0, esz = 1; int C = 0, HW = 0;
    if (!strcmp(name, "route1")) { src = t->r1; total = N * 32 * 1024; C = 32; HW = 1024; }
    else if (!strcmp(name, "route2")) { src = t->r2; total = N * 64 * 256; C = 64; HW = 256; }
    else if (!strcmp(name, "route3")) { src = t->r3; total = N * VFC1_K; }
    else if (!strcmp(name, "fc1_mask")) { src = t->relu1; total = N * VFC1_N; }
    else if (!strcmp(name, "fc_keep")) { src = t->keep1; total = N * VFC1_N; }
    else if (!strcmp(name, "cls_mask")) { src = t->reluc; total = B * VHID; }
    else if (!strcmp(name, "cls_keep")) { src = t->keepc; total = B * VHID; }
    else if (!strcmp(name, "e1")) { src = t->emb; total = B * E; esz = 4; }
    else if (!strcmp(name, "e2")) { src = t->emb + B * E; total = B * E; esz = 4; }
    else if (!strcmp(name, "similarity")) { src = t->sim; total = B; esz = 4; }
    else if (!strcmp(name, "distance")) { src = t->dist; total = B; esz = 4; }
    else return FAIL(SIGGAN_E_ARG, "siggan_verifier_train_debug: unknown stage '%s'", name);
    if (n != total) return FAIL(SIGGAN_E_ARG, "siggan_verifier_train_debug: '%s' holds %lld elements, caller asked for %lld", name,
                                 (long long)total, (long long)n);
    DevGuard dg(t->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    if (C) {
        hipLaunchKernelGGL(k_nchw<uint8_t>, dim3(blocks(total)), dim3(256), 0, s, (const uint8_t*)src, (uint8_t*)out, total, C, HW);
        return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_train_debug: kernel launch failed");
    }
    HIPCHK(hipMemcpyAsync(out, src, (size_t)(total * esz), hipMemcpyDeviceToDevice, s));
    return SIGGAN_OK;
}
