// verifier.hip -- eval-mode forward of the Siamese signature verifier (include/siggan_verifier.h; the reference's
// signature_verifier_eval.py:39-179).  gfx950 only, fp32 only, NHWC inside the library.
//
// One score call is six launches:
//   k_vconv1   direct 5x5 stencil (Cin = 1) on fp32 or uint8 images; folded conv-bias + BatchNorm affine, ReLU and the
//              2x2 max before the store: the 64x64x32 pre-pool tensor never exists.
//   k_vconv    stride-1 implicit GEMM on v_mfma_f32_32x32x2_f32 (conv2: 25 taps, conv3: 9 taps).  The GEMM's M rows are
//              ordered (n, ph, pw, dy, dx): the four pixels of a pooling window are four consecutive rows aligned to 4,
//              which in the 32x32 C/D layout are registers 4g..4g+3 of ONE lane -- the max is taken in registers and only
//              the pooled tensor is stored.
//   k_vfc1     (N x 8192) . (8192 x 512) on the same MFMA, K always split in VFC1_SPLIT slices (16 MB of weights
//              dominate at small N; the split does not depend on N, so a row's sum order depends neither on its position
//              in the batch nor on the batch).  Partials go to the workspace.
//   k_vtail    per embedding row: sum the K slices in order + bias + ReLU (fc1), fc2, L2 normalise.
//   k_vhead    per pair: |e1 - e2| -> Linear(E,64) + ReLU -> Linear(64,1) -> sigmoid.
// No atomics, no host synchronisation; every sum has a fixed order, so equal images give equal bits.
//
// siggan_verifier_input_grad (include/siggan_verifier_grad.h) is 16 launches: the five encoder launches in their REC form (one
// route byte per pooled element, the row norms), k_vhead_grad, k_vemb_bwd, k_tgemm (d pool3 = dh . Wfc1), and per conv layer
// k_vunpool + the input gradient (k_tconv over the flipped packs of k_vflip for conv3 / conv2, k_vconv1_dgrad for conv1).
//
// siggan_verifier_pairs (include/siggan_verifier_pairs.h) is k_vpairs (+ k_vpairs_best for the row maxima) of verifier_pairs.h.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <algorithm>
#include <new>

#include "../../include/siggan_verifier.h"
#include "../../include/siggan_verifier_grad.h"
#include "../../include/siggan_verifier_pairs.h"
#include "../../include/siggan_verifier_topk.h"
#include "host.h"
#include "verifier_parts.h"
#include "verifier_pairs.h"

using namespace siggan;

namespace {

// ---------------------------------------------------------------- bind-time packing
// scale = gamma / sqrt(var + eps); shift = (conv_bias - mean) * scale + beta
__global__ void k_vfold(const float* __restrict__ cb, const float* __restrict__ g, const float* __restrict__ b,
                        const float* __restrict__ rm, const float* __restrict__ rv, float eps, float* __restrict__ sc,
                        float* __restrict__ sh, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float s = g[c] / sqrtf(rv[c] + eps);
    sc[c] = s;
    sh[c] = (cb[c] - rm[c]) * s + b[c];
}
// torch (Co, Ci, T) -> [Co][t * Ci + ci]
__global__ void k_vpack_conv(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int T) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Co * Ci * T) return;
    const int ci = (int)(i % Ci), t = (int)((i / Ci) % T), co = (int)(i / ((int64_t)Ci * T));
    wp[i] = w[((int64_t)co * Ci + ci) * T + t];
}
// fc1.weight columns from torch's (c, h, w) flatten order to the pooled activation's (h, w, c) order
__global__ void k_vpack_fc1(const float* __restrict__ w, float* __restrict__ wp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)VFC1_N * VFC1_K) return;
    const int k = (int)(i % VFC1_K), j = (int)(i / VFC1_K);
    const int c = k & 127, hw = k >> 7;
    wp[i] = w[(int64_t)j * VFC1_K + c * 64 + hw];
}

// ---------------------------------------------------------------- conv1 + affine + ReLU + pool
// Which element of a pooling window (v in (dy, dx) order) its gradient goes to: the first of equal maxima, 4 when the maximum
// is not positive (ReLU passes nothing) -- torch's rules, as k_bnpool in the trainer.
__device__ __forceinline__ uint8_t pool_route(const float (&v)[4]) {
    float best = v[0];
    int idx = 0;
#pragma unroll
    for (int e = 1; e < 4; ++e)
        if (v[e] > best) { best = v[e]; idx = e; }
    return best > 0.f ? (uint8_t)idx : (uint8_t)4;
}
// thread = (pooled pixel, 8 output channels); block = 64 pooled pixels x 4 channel groups.  Images [0, nsplit) come from
// x1, the rest from x2.  out: (N, 32, 32, 32) NHWC.  REC (siggan_verifier_input_grad): one route byte per pooled element beside it.
template <bool U8, bool REC>
__global__ __launch_bounds__(256) void k_vconv1(const void* __restrict__ x1, const void* __restrict__ x2, int nsplit,
                                                const float* __restrict__ w /* (32, 25) */, const float* __restrict__ sc,
                                                const float* __restrict__ sh, float* __restrict__ out, uint8_t* __restrict__ route) {
    __shared__ float sW[25][32];
    const int tid = threadIdx.x;
    for (int i = tid; i < 800; i += 256) sW[i % 25][i / 25] = w[i];
    __syncthreads();
    const int cg = tid & 3;
    const int64_t P = (int64_t)blockIdx.x * 64 + (tid >> 2);
    const int n = (int)(P >> 10), ph = (int)(P >> 5) & 31, pw = (int)P & 31;
    const void* img = vimage<U8>(x1, x2, nsplit, n);
    float patch[6][6];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const int iy = 2 * ph - 2 + r, ix = 2 * pw - 2 + c;
            patch[r][c] = (iy >= 0 && iy < VS && ix >= 0 && ix < VS) ? vload<U8>(img, iy * VS + ix) : 0.f;
        }
    float acc[4][8];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[p][c] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            float wv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) wv[c] = sW[ky * 5 + kx][cg * 8 + c];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float xv = patch[(p >> 1) + ky][(p & 1) + kx];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[p][c] = fmaf(xv, wv[c], acc[p][c]);
            }
        }
    float* o = out + (size_t)P * 32 + cg * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float s = sc[cg * 8 + c], t = sh[cg * 8 + c];
        float m = 0.f;                                                 // ReLU: max(0, .) commutes with the window max
#pragma unroll
        for (int p = 0; p < 4; ++p) m = fmaxf(m, fmaf(acc[p][c], s, t));
        o[c] = m;
        if (REC) {
            float v[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) v[p] = fmaf(acc[p][c], s, t);
            route[(size_t)P * 32 + cg * 8 + c] = pool_route(v);
        }
    }
}

// ---------------------------------------------------------------- conv2 / conv3: implicit GEMM + affine + ReLU + pool
// x: (N, H, H, CI) NHWC; wp: [CO][KS*KS*CI]; out: (N, H/2, H/2, CO).  conv_tile's 128 x 64 block tile over rows in pooling-window
// order (PoolRows): registers 4g..4g+3 of an accumulator are one window, so the max is taken in registers.
template <int KS, int CI, int CO, int H, bool REC>
__global__ __launch_bounds__(256) void k_vconv(const float* __restrict__ x, const float* __restrict__ wp,
                                               const float* __restrict__ sc, const float* __restrict__ sh,
                                               float* __restrict__ out, uint8_t* __restrict__ route) {
    constexpr int BM = 128, BN = 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    f32x16 acc[2];
    conv_tile<KS, CI, CO, H, BN, PoolRows>(x, wp, m0, n0, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int co = n0 + 32 * j + li;
        const float s = sc[co], t = sh[co];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float mx = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fmaf(acc[j][4 * g + e], s, t));
            const int64_t pq = (m0 + wave * 32 + 8 * g + 4 * lh) >> 2;
            out[(size_t)pq * CO + co] = mx;
            if (REC) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaf(acc[j][4 * g + e], s, t);
                route[(size_t)pq * CO + co] = pool_route(v);
            }
        }
    }
}

// ---------------------------------------------------------------- fc1: split-K partial products
// A (M, 8192) row-major (pool3, h-w-c order); W packed (512, 8192); part [VFC1_SPLIT][M][512].  64 x 64 tiles, four waves of
// 32 x 32; grid (8, ceil(M / 64), VFC1_SPLIT).  Rows >= M are staged as zeros and never stored.
__global__ __launch_bounds__(256) void k_vfc1(const float* __restrict__ A, const float* __restrict__ W,
                                              float* __restrict__ part, int M) {
    constexpr int BK = 32, LD = 64 + 4;
    __shared__ float sA[BK][LD], sB[BK][LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, kb = blockIdx.z * VFC1_KS;
    const int row = tid & 63, qd = tid >> 6;
    const bool av = m0 + row < M;
    const float* ap = A + (size_t)(av ? m0 + row : 0) * VFC1_K + kb + qd * 8;
    const float* bp = W + (size_t)(n0 + row) * VFC1_K + kb + qd * 8;
    f32x4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            ra[j] = av ? *reinterpret_cast<const f32x4*>(ap + k0 + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
            rb[j] = *reinterpret_cast<const f32x4*>(bp + k0 + 4 * j);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < VFC1_KS; k0 += BK) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sA[qd * 8 + 4 * j + e][row] = ra[j][e];
                sB[qd * 8 + 4 * j + e][row] = rb[j][e];
            }
        __syncthreads();
        if (k0 + BK < VFC1_KS) fetch(k0 + BK);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[2 * s + lh][wm * 32 + li], sB[2 * s + lh][wn * 32 + li], acc, 0, 0, 0);
        __syncthreads();
    }
    float* pz = part + (size_t)blockIdx.z * M * VFC1_N;
    const int nn = n0 + wn * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int mm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (mm < M) pz[(size_t)mm * VFC1_N + nn] = acc[r];
    }
}

// ---------------------------------------------------------------- tail: fc1 finish, fc2, L2 normalise (one block per row)
// rows [0, nsplit) are written to out1, the rest to out2 (row - nsplit)
__global__ __launch_bounds__(256) void k_vtail(const float* __restrict__ part, int M, const float* __restrict__ b1,
                                               const float* __restrict__ w2 /* (E, 512) */, const float* __restrict__ b2, int E,
                                               float* __restrict__ fc1, float* __restrict__ out1, float* __restrict__ out2,
                                               int nsplit, float* __restrict__ nrm_out /* (M) or null */) {
    extern __shared__ float se[];                      // E embedding entries
    __shared__ float sh1[VFC1_N];
    const int row = blockIdx.x, tid = threadIdx.x;
    for (int j = tid; j < VFC1_N; j += 256) {
        const float a = fc1_finish(part, M, row, j, b1);
        sh1[j] = a;
        fc1[(size_t)row * VFC1_N + j] = a;
    }
    const float nrm = fc2_norm(sh1, w2, b2, E, se);
    float* o = row < nsplit ? out1 + (size_t)row * E : out2 + (size_t)(row - nsplit) * E;
    for (int i = tid; i < E; i += 256) o[i] = se[i] / nrm;
    if (nrm_out && tid == 0) nrm_out[row] = nrm;
}

// ---------------------------------------------------------------- pair head (one 64-thread block per pair)
// sd [E] = |e1 - e2| in LDS (written and synchronised by the caller) -> the similarity; a = thread j's hidden unit after ReLU
__device__ __forceinline__ float head_score(const float* sd, int E, const float* __restrict__ w0, const float* __restrict__ b0,
                                            const float* __restrict__ w3, const float* __restrict__ b3, float& a) {
    const int j = threadIdx.x;
    const float* wr = w0 + (size_t)j * E;
    a = 0.f;
    for (int k = 0; k < E; ++k) a = fmaf(sd[k], wr[k], a);
    a = head_hidden(a, b0[j]);
    return head_sigmoid(wave_sum(a * w3[j]), b3[0]);
}
__global__ __launch_bounds__(64) void k_vhead(const float* __restrict__ e1, const float* __restrict__ e2, int E,
                                              const float* __restrict__ w0 /* (64, E) */, const float* __restrict__ b0,
                                              const float* __restrict__ w3 /* (64) */, const float* __restrict__ b3,
                                              float* __restrict__ score) {
    extern __shared__ float sd[];                      // E differences
    const int p = blockIdx.x, j = threadIdx.x;
    for (int k = j; k < E; k += VHID) sd[k] = fabsf(e1[(size_t)p * E + k] - e2[(size_t)p * E + k]);
    __syncthreads();
    float a;
    const float s = head_score(sd, E, w0, b0, w3, b3, a);
    if (j == 0) score[p] = s;
}

// ---------------------------------------------------------------- siggan_verifier_input_grad: head forward + backward
// One 64-thread block per image: the head of k_vhead on |e - r| (the same expression: score is siggan_verifier_compare's bits),
// the two terms, and d objective / d e into de.  r is a constant.
//   embed  0.5 * sum_k (e - r)^2:            d/de = e - r
//   score  -max(log s, -100):                d/dlogit = (s - 1) / max((1 - s) s, 1e-12) * (s (1 - s)), then classifier.3,
//          the hidden ReLU's mask, classifier.0 and |u|' = sign(u) with sign(0) = 0
// terms [2][N] unweighted, a term whose weight is 0 is not formed and reported as 0.
__global__ __launch_bounds__(64) void k_vhead_grad(const float* __restrict__ emb, const float* __restrict__ ref, int N, int E,
                                                   const float* __restrict__ w0, const float* __restrict__ b0,
                                                   const float* __restrict__ w3, const float* __restrict__ b3, float we, float ws,
                                                   float* __restrict__ de, float* __restrict__ objective, float* __restrict__ terms,
                                                   float* __restrict__ score, uint8_t* __restrict__ cls_mask,
                                                   int8_t* __restrict__ diff_sign) {
    extern __shared__ float sd[];                      // E |differences|
    __shared__ float sdh[VHID];
    const int p = blockIdx.x, j = threadIdx.x;
    float q = 0.f;
    for (int k = j; k < E; k += VHID) {
        const float d = emb[(size_t)p * E + k] - ref[(size_t)p * E + k];
        sd[k] = fabsf(d);
        diff_sign[(size_t)p * E + k] = d > 0.f ? 1 : (d < 0.f ? -1 : 0);
        q = fmaf(d, d, q);
    }
    __syncthreads();
    const float te = we > 0.f ? 0.5f * wave_sum(q) : 0.f;
    float a;
    const float s = head_score(sd, E, w0, b0, w3, b3, a);
    const float ts = ws > 0.f ? -fmaxf(logf(s), -100.f) : 0.f;
    const float dlogit = ws > 0.f ? ws * ((s - 1.0f) / fmaxf((1.0f - s) * s, 1e-12f) * (s * (1.0f - s))) : 0.f;
    cls_mask[(size_t)p * VHID + j] = a > 0.f;
    sdh[j] = a > 0.f ? dlogit * w3[j] : 0.f;
    if (j == 0) {
        float obj = 0.f;
        if (we > 0.f) obj += we * te;
        if (ws > 0.f) obj += ws * ts;
        objective[p] = obj;
        if (terms) { terms[p] = te; terms[N + p] = ts; }
        if (score) score[p] = s;
    }
    __syncthreads();
    for (int k = j; k < E; k += VHID) {
        const float d = emb[(size_t)p * E + k] - ref[(size_t)p * E + k];
        float g = 0.f;
        if (ws > 0.f) {
            float da = 0.f;
            for (int i = 0; i < VHID; ++i) da = fmaf(sdh[i], w0[(size_t)i * E + k], da);
            g = d > 0.f ? da : (d < 0.f ? -da : 0.f);
        }
        de[(size_t)p * E + k] = we > 0.f ? fmaf(we, d, g) : g;
    }
}

// ---------------------------------------------------------------- per row: normalise / fc2 / fc1 ReLU backward (256 threads)
// F.normalize: d(raw) = (de - e (e . de)) / max(||raw||, 1e-12) (nrm is k_vtail's, already clamped); dh = fc2^T d(raw) where the
// stored fc1 output is > 0.
__global__ __launch_bounds__(256) void k_vemb_bwd(const float* __restrict__ de, int E, const float* __restrict__ emb,
                                                  const float* __restrict__ nrm_in, const float* __restrict__ w2 /* (E, 512) */,
                                                  const float* __restrict__ fc1, float* __restrict__ dh,
                                                  uint8_t* __restrict__ fc1_mask) {
    extern __shared__ float sg[];                      // E raw-embedding gradients
    __shared__ float sred[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float nrm = nrm_in[row];
    float dot = 0.f;
    for (int k = tid; k < E; k += 256) dot = fmaf(de[(size_t)row * E + k], emb[(size_t)row * E + k], dot);
    dot = wave_sum(dot);
    if (lane == 0) sred[wave] = dot;
    __syncthreads();
    dot = (sred[0] + sred[1]) + (sred[2] + sred[3]);
    for (int k = tid; k < E; k += 256) sg[k] = (de[(size_t)row * E + k] - emb[(size_t)row * E + k] * dot) / nrm;
    __syncthreads();
    for (int j = tid; j < VFC1_N; j += 256) {
        float a = 0.f;
        for (int o = 0; o < E; ++o) a = fmaf(sg[o], w2[(size_t)o * VFC1_N + j], a);
        const bool on = fc1[(size_t)row * VFC1_N + j] > 0.f;
        dh[(size_t)row * VFC1_N + j] = on ? a : 0.f;
        fc1_mask[(size_t)row * VFC1_N + j] = on;
    }
}

// ---------------------------------------------------------------- un-pool through ReLU and the folded BatchNorm affine
// thread = pooled element (q, c), writes its four pixels: dy[n, y, x, c] = route matches (y & 1, x & 1) ? dpool * scale[c] : 0
__global__ void k_vunpool(const float* __restrict__ dpool, const uint8_t* __restrict__ route, const float* __restrict__ sc, int C,
                          int H, int64_t total, float* __restrict__ dy) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C), HP = H / 2;
    const int64_t q = i / C;
    const int pw = (int)(q % HP), ph = (int)((q / HP) % HP);
    const int64_t n = q / (HP * HP);
    const int r = route[i];
    const float g = dpool[i] * sc[c];
#pragma unroll
    for (int e = 0; e < 4; ++e)
        dy[((size_t)(n * H + 2 * ph + (e >> 1)) * H + 2 * pw + (e & 1)) * C + c] = r == e ? g : 0.f;
}

// ---------------------------------------------------------------- conv1 input gradient (32 -> 1 channel, 5 x 5)
// dx[n, y, x] = sum_{ky, kx, c} dy[n, y + 2 - ky, x + 2 - kx, c] * w[c][ky][kx].  Block = one image row (64 pixels), four lanes
// per pixel with 8 channels each; taps in order, then the four lanes by a two-step butterfly: one fixed order.
__global__ __launch_bounds__(256) void k_vconv1_dgrad(const float* __restrict__ dy /* (N, 64, 64, 32) */,
                                                      const float* __restrict__ w /* (32, 25) */, float* __restrict__ dx) {
    __shared__ float sW[25][32];
    const int tid = threadIdx.x;
    for (int i = tid; i < 800; i += 256) sW[i % 25][i / 25] = w[i];
    __syncthreads();
    const int cg = tid & 3;
    const int64_t P = (int64_t)blockIdx.x * 64 + (tid >> 2);
    const int64_t n = P >> 12;
    const int py = (int)(P >> 6) & 63, px = (int)P & 63;
    const float* img = dy + (size_t)n * VS * VS * 32 + cg * 8;
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < 5; ++ky)
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
            const int iy = py + 2 - ky, ix = px + 2 - kx;
            if (iy >= 0 && iy < VS && ix >= 0 && ix < VS) {
                const float* src = img + ((size_t)iy * VS + ix) * 32;
                const f32x4 g0 = *reinterpret_cast<const f32x4*>(src), g1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fmaf(g0[c], sW[ky * 5 + kx][cg * 8 + c], acc);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc = fmaf(g1[c], sW[ky * 5 + kx][cg * 8 + 4 + c], acc);
            }
        }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    if (cg == 0) dx[P] = acc;
}

// packed forward weights [Co][t * Ci + ci] -> the input gradient's flipped pack [Ci][(T - 1 - t) * Co + co] (k_tpack's layout)
__global__ void k_vflip(const float* __restrict__ wp, float* __restrict__ flip, int Co, int Ci, int T) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Co * Ci * T) return;
    const int ci = (int)(i % Ci), t = (int)((i / Ci) % T), co = (int)(i / ((int64_t)Ci * T));
    flip[((int64_t)ci * T + (T - 1 - t)) * Co + co] = wp[i];
}

}  // namespace

struct siggan_verifier {
    int device, E, Nmax;
    bool bound;
    int last_n;                          // images of the last embed / score call (0: none yet)
    char* ws;
    // packs (filled by bind)
    float *w1, *sc1, *sh1, *wp2, *sc2, *sh2, *wp3, *sc3, *sh3, *wfc1, *bfc1, *wfc2, *bfc2, *wc0, *bc0, *wc3, *bc3;
    // activations
    float *pool1, *pool2, *pool3, *part, *fc1, *emb;
    // siggan_verifier_input_grad (allocated by _enable; gws null before)
    char* gws;
    int grad_n;                          // images of the last input_grad call (0: none yet)
    float *wf2, *wf3;                    // flipped packs [Ci][(T - 1 - t) * Co + co]
    uint8_t *r1, *r2, *r3, *fc1_mask, *cls_mask;
    int8_t* diff_sign;
    float *nrm, *de, *dh, *dp1, *dy1, *dp2, *dy2, *dp3, *dy3;   // dp3, dy3, dp2, dy2 share dy1's bytes (dead before it is written)
    // siggan_verifier_pairs (allocated by _enable; pws null before)
    char* pws;
    int pair_max, pair_kp;               // query rows the key workspace holds; E rounded up to PBK
    float* wpk;                          // classifier.0.weight in the B operand's lane order (k_vpairs_pack)
    unsigned long long* pkeys;           // [pair_max][PSPLIT_MAX][2]
    // siggan_verifier_pairs_topk (allocated by _topk_enable; tkeys null before)
    unsigned long long* tkeys;           // [topk_max][PSPLIT_MAX][2][topk_k]
    int topk_max, topk_k;
};

extern "C" int siggan_verifier_create(int32_t device, int32_t E, int32_t max_images, siggan_verifier** out) {
    if (!out) return FAIL(SIGGAN_E_ARG, "siggan_verifier_create: null argument");
    *out = nullptr;
    if (E < 1 || E > SIGGAN_VERIFIER_MAX_EMBEDDING)
        return FAIL(SIGGAN_E_ARG, "embedding_dim %d outside [1, %d]", E, SIGGAN_VERIFIER_MAX_EMBEDDING);
    if (max_images < 1 || max_images > 8192) return FAIL(SIGGAN_E_ARG, "max_images %d outside [1, 8192]", max_images);
    DevGuard dg(device); HIPCHK(dg.err);
    siggan_verifier* v = new (std::nothrow) siggan_verifier();
    if (!v) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    v->device = device; v->E = E; v->Nmax = max_images; v->bound = false; v->last_n = 0; v->ws = nullptr; v->gws = nullptr; v->grad_n = 0;
    v->pws = nullptr; v->pair_max = 0; v->pair_kp = 0;
    v->tkeys = nullptr; v->topk_max = 0; v->topk_k = 0;
    const int64_t N = max_images;
    size_t off = 0; char* base = nullptr;
    auto carve = [&](float** p, int64_t n) { if (base) *p = (float*)(base + off); off += ((size_t)n * 4 + 255) & ~(size_t)255; };
    for (int pass = 0; pass < 2; ++pass) {
        off = 0;
        carve(&v->w1, 32 * 25); carve(&v->sc1, 32); carve(&v->sh1, 32);
        carve(&v->wp2, 64 * 25 * 32); carve(&v->sc2, 64); carve(&v->sh2, 64);
        carve(&v->wp3, 128 * 9 * 64); carve(&v->sc3, 128); carve(&v->sh3, 128);
        carve(&v->wfc1, (int64_t)VFC1_N * VFC1_K); carve(&v->bfc1, VFC1_N);
        carve(&v->wfc2, (int64_t)E * VFC1_N); carve(&v->bfc2, E);
        carve(&v->wc0, (int64_t)VHID * E); carve(&v->bc0, VHID); carve(&v->wc3, VHID); carve(&v->bc3, 1);
        carve(&v->pool1, N * 32 * 32 * 32); carve(&v->pool2, N * 16 * 16 * 64); carve(&v->pool3, N * VFC1_K);
        carve(&v->part, N * VFC1_SPLIT * VFC1_N); carve(&v->fc1, N * VFC1_N); carve(&v->emb, N * E);
        if (pass == 0) {
            hipError_t e = hipMalloc((void**)&base, off);
            if (e != hipSuccess) { delete v; return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", off, hipGetErrorString(e)); }
            v->ws = base;
        }
    }
    *out = v;
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_destroy(siggan_verifier* v) {
    if (!v) return SIGGAN_OK;
    DevGuard dg(v->device);
    (void)hipDeviceSynchronize();
    if (v->ws) (void)hipFree(v->ws);
    if (v->gws) (void)hipFree(v->gws);
    if (v->pws) (void)hipFree(v->pws);
    if (v->tkeys) (void)hipFree(v->tkeys);
    delete v;
    return SIGGAN_OK;
}

static void flip_packs(siggan_verifier* v, hipStream_t s) {
    hipLaunchKernelGGL(k_vflip, dim3(blocks(64 * 32 * 25)), dim3(256), 0, s, (const float*)v->wp2, v->wf2, 64, 32, 25);
    hipLaunchKernelGGL(k_vflip, dim3(blocks(128 * 64 * 9)), dim3(256), 0, s, (const float*)v->wp3, v->wf3, 128, 64, 9);
}

static void pairs_pack(siggan_verifier* v, hipStream_t s) {
    hipLaunchKernelGGL(k_vpairs_pack, dim3(blocks((int64_t)v->pair_kp * VHID)), dim3(256), 0, s, (const float*)v->wc0, v->E, v->pair_kp, v->wpk);
}

extern "C" int siggan_verifier_bind(siggan_verifier* v, const siggan_verifier_weights* w, void* stream) {
    if (!v || !w) return FAIL(SIGGAN_E_ARG, "siggan_verifier_bind: null argument");
    const float* const* p = reinterpret_cast<const float* const*>(w);
    for (int i = 0; i < 26; ++i)
        if (!p[i]) return FAIL(SIGGAN_E_ARG, "siggan_verifier_bind: weight pointer %d is null", i);
    if (!(w->bn_eps > 0.f)) return FAIL(SIGGAN_E_ARG, "siggan_verifier_bind: bn_eps must be positive");
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    const int E = v->E;
    auto copy = [&](float* dst, const float* src, int64_t n) { return hipMemcpyAsync(dst, src, (size_t)n * 4, hipMemcpyDeviceToDevice, s); };
    HIPCHK(copy(v->w1, w->conv1_weight, 800));
    HIPCHK(copy(v->bfc1, w->fc1_bias, VFC1_N));
    HIPCHK(copy(v->wfc2, w->fc2_weight, (int64_t)E * VFC1_N));
    HIPCHK(copy(v->bfc2, w->fc2_bias, E));
    HIPCHK(copy(v->wc0, w->cls0_weight, (int64_t)VHID * E));
    HIPCHK(copy(v->bc0, w->cls0_bias, VHID));
    HIPCHK(copy(v->wc3, w->cls3_weight, VHID));
    HIPCHK(copy(v->bc3, w->cls3_bias, 1));
    hipLaunchKernelGGL(k_vfold, dim3(1), dim3(128), 0, s, w->conv1_bias, w->bn1_weight, w->bn1_bias, w->bn1_running_mean,
                       w->bn1_running_var, w->bn_eps, v->sc1, v->sh1, 32);
    hipLaunchKernelGGL(k_vfold, dim3(1), dim3(128), 0, s, w->conv2_bias, w->bn2_weight, w->bn2_bias, w->bn2_running_mean,
                       w->bn2_running_var, w->bn_eps, v->sc2, v->sh2, 64);
    hipLaunchKernelGGL(k_vfold, dim3(1), dim3(128), 0, s, w->conv3_bias, w->bn3_weight, w->bn3_bias, w->bn3_running_mean,
                       w->bn3_running_var, w->bn_eps, v->sc3, v->sh3, 128);
    hipLaunchKernelGGL(k_vpack_conv, dim3(blocks(64 * 32 * 25)), dim3(256), 0, s, w->conv2_weight, v->wp2, 64, 32, 25);
    hipLaunchKernelGGL(k_vpack_conv, dim3(blocks(128 * 64 * 9)), dim3(256), 0, s, w->conv3_weight, v->wp3, 128, 64, 9);
    hipLaunchKernelGGL(k_vpack_fc1, dim3(blocks((int64_t)VFC1_N * VFC1_K)), dim3(256), 0, s, w->fc1_weight, v->wfc1);
    if (v->gws) flip_packs(v, s);
    if (v->pws) pairs_pack(v, s);
    if (hipGetLastError() != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_verifier_bind: kernel launch failed");
    v->bound = true;
    return SIGGAN_OK;
}

// the encoder over n images (the first nsplit from x1, the rest from x2); embeddings to out1 / out2 likewise.  REC (fp32 images):
// the same five launches with the route bytes and the rows' norms recorded for siggan_verifier_input_grad.
template <bool REC>
static int encode(siggan_verifier* v, const void* x1, const void* x2, int fmt, int n, int nsplit, float* out1, float* out2,
                  hipStream_t s) {
    uint8_t* const none = nullptr;
    if (fmt == SIGGAN_VFMT_U8)
        hipLaunchKernelGGL((k_vconv1<true, false>), dim3(n * 16), dim3(256), 0, s, x1, x2, nsplit, v->w1, v->sc1, v->sh1, v->pool1, none);
    else
        hipLaunchKernelGGL((k_vconv1<false, REC>), dim3(n * 16), dim3(256), 0, s, x1, x2, nsplit, v->w1, v->sc1, v->sh1, v->pool1,
                           REC ? v->r1 : none);
    hipLaunchKernelGGL((k_vconv<5, 32, 64, 32, REC>), dim3(n * 1024 / 128, 1), dim3(256), 0, s, v->pool1, v->wp2, v->sc2, v->sh2, v->pool2,
                       REC ? v->r2 : none);
    hipLaunchKernelGGL((k_vconv<3, 64, 128, 16, REC>), dim3(n * 256 / 128, 2), dim3(256), 0, s, v->pool2, v->wp3, v->sc3, v->sh3, v->pool3,
                       REC ? v->r3 : none);
    hipLaunchKernelGGL(k_vfc1, dim3(VFC1_N / 64, (n + 63) / 64, VFC1_SPLIT), dim3(256), 0, s, v->pool3, v->wfc1, v->part, n);
    hipLaunchKernelGGL(k_vtail, dim3(n), dim3(256), (size_t)v->E * 4, s, v->part, n, v->bfc1, v->wfc2, v->bfc2, v->E, v->fc1, out1,
                       out2, nsplit, REC ? v->nrm : (float*)nullptr);
    v->last_n = n;
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "verifier encoder: kernel launch failed");
}
static int head(siggan_verifier* v, const float* e1, const float* e2, int np, float* score, hipStream_t s) {
    hipLaunchKernelGGL(k_vhead, dim3(np), dim3(VHID), (size_t)v->E * 4, s, e1, e2, v->E, v->wc0, v->bc0, v->wc3, v->bc3, score);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "verifier head: kernel launch failed");
}
static int vcheck(const siggan_verifier* v, const char* fn) {
    if (!v) return FAIL(SIGGAN_E_ARG, "%s: null context", fn);
    if (!v->bound) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_bind has not been called", fn);
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_embed(siggan_verifier* v, const void* x, int32_t fmt, int32_t n, float* emb, void* stream) {
    int rc = vcheck(v, "siggan_verifier_embed"); if (rc) return rc;
    if (!x || !emb) return FAIL(SIGGAN_E_ARG, "siggan_verifier_embed: null tensor");
    if (fmt != SIGGAN_VFMT_F32 && fmt != SIGGAN_VFMT_U8) return FAIL(SIGGAN_E_ARG, "siggan_verifier_embed: unknown fmt %d", fmt);
    if (n < 1 || n > v->Nmax) return FAIL(SIGGAN_E_ARG, "siggan_verifier_embed: n_images %d outside [1, max_images=%d]", n, v->Nmax);
    DevGuard dg(v->device); HIPCHK(dg.err);
    return encode<false>(v, x, x, fmt, n, n, emb, emb, (hipStream_t)stream);
}

extern "C" int siggan_verifier_compare(siggan_verifier* v, const float* e1, const float* e2, int32_t np, float* score, void* stream) {
    int rc = vcheck(v, "siggan_verifier_compare"); if (rc) return rc;
    if (!e1 || !e2 || !score) return FAIL(SIGGAN_E_ARG, "siggan_verifier_compare: null tensor");
    if (np < 1) return FAIL(SIGGAN_E_ARG, "siggan_verifier_compare: n_pairs %d < 1", np);
    DevGuard dg(v->device); HIPCHK(dg.err);
    return head(v, e1, e2, np, score, (hipStream_t)stream);
}

extern "C" int siggan_verifier_score(siggan_verifier* v, const void* x1, const void* x2, int32_t fmt, int32_t np, float* e1,
                                     float* e2, float* score, void* stream) {
    int rc = vcheck(v, "siggan_verifier_score"); if (rc) return rc;
    if (!x1 || !x2 || !score) return FAIL(SIGGAN_E_ARG, "siggan_verifier_score: null tensor");
    if (fmt != SIGGAN_VFMT_F32 && fmt != SIGGAN_VFMT_U8) return FAIL(SIGGAN_E_ARG, "siggan_verifier_score: unknown fmt %d", fmt);
    if (np < 1 || 2 * (int64_t)np > v->Nmax)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_score: 2 * n_pairs = %lld outside [2, max_images=%d]", 2 * (long long)np, v->Nmax);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    float* o1 = e1 ? e1 : v->emb;
    float* o2 = e2 ? e2 : v->emb + (size_t)np * v->E;
    if ((rc = encode<false>(v, x1, x2, fmt, 2 * np, np, o1, o2, s))) return rc;
    return head(v, o1, o2, np, score, s);
}

extern "C" int siggan_verifier_debug_tensor(siggan_verifier* v, const char* name, float* out, int64_t n, void* stream) {
    int rc = vcheck(v, "siggan_verifier_debug_tensor"); if (rc) return rc;
    if (!name || !out) return FAIL(SIGGAN_E_ARG, "siggan_verifier_debug_tensor: null argument");
    if (v->last_n < 1) return FAIL(SIGGAN_E_ARG, "siggan_verifier_debug_tensor: no embed / score call yet");
    const float* src; int C, HW;
    if (!strcmp(name, "pool1")) { src = v->pool1; C = 32; HW = 1024; }
    else if (!strcmp(name, "pool2")) { src = v->pool2; C = 64; HW = 256; }
    else if (!strcmp(name, "pool3")) { src = v->pool3; C = 128; HW = 64; }
    else if (!strcmp(name, "fc1")) { src = v->fc1; C = VFC1_N; HW = 1; }
    else return FAIL(SIGGAN_E_ARG, "siggan_verifier_debug_tensor: unknown tensor '%s'", name);
    const int64_t total = (int64_t)v->last_n * C * HW;
    if (n != total) return FAIL(SIGGAN_E_ARG, "siggan_verifier_debug_tensor: '%s' holds %lld floats, caller asked for %lld", name,
                                 (long long)total, (long long)n);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_nchw<float>, dim3(blocks(total)), dim3(256), 0, (hipStream_t)stream, src, out, total, C, HW);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_debug_tensor: kernel launch failed");
}

// ---------------------------------------------------------------- siggan_verifier_input_grad
// The backward workspace, per image of max_images: route planes 32768 + 16384 + 8192 B, dp1 131072 B, dy1 524288 B (whose bytes
// first hold dp3, dy3, dp2 and dy2: 491520 B, all dead before the conv1 un-pool writes dy1), dh 2048 B, de 4 E B, the two masks,
// the diff signs and the norm: 715332 + 5 E bytes -- about 0.70 MB -- plus the two flipped packs (500 KB) once.
extern "C" int siggan_verifier_input_grad_enable(siggan_verifier* v) {
    if (!v) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad_enable: null context");
    if (v->gws) return SIGGAN_OK;
    DevGuard dg(v->device); HIPCHK(dg.err);
    const int64_t N = v->Nmax, E = v->E;
    size_t off = 0; char* base = nullptr;
    auto carve = [&](void* pp, int64_t bytes) { if (base) *(void**)pp = (void*)(base + off); off += ((size_t)bytes + 255) & ~(size_t)255; };
    for (int pass = 0; pass < 2; ++pass) {
        off = 0;
        carve(&v->wf2, 51200 * 4); carve(&v->wf3, 73728 * 4);
        carve(&v->r1, N * 32768); carve(&v->r2, N * 16384); carve(&v->r3, N * VFC1_K);
        carve(&v->fc1_mask, N * VFC1_N); carve(&v->cls_mask, N * VHID); carve(&v->diff_sign, N * E);
        carve(&v->nrm, N * 4); carve(&v->de, N * E * 4); carve(&v->dh, N * VFC1_N * 4);
        carve(&v->dp1, N * 32768 * 4); carve(&v->dy1, N * 131072 * 4);
        if (pass == 0) {
            hipError_t e = hipMalloc((void**)&base, off);
            if (e != hipSuccess) return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", off, hipGetErrorString(e));
        }
    }
    v->dp3 = v->dy1;                     // N * 8192
    v->dy3 = v->dp3 + N * 8192;          // N * 32768
    v->dp2 = v->dy3 + N * 32768;         // N * 16384
    v->dy2 = v->dp2 + N * 16384;         // N * 65536: ends at N * 122880 <= N * 131072
    v->gws = base;
    if (v->bound) {                      // a set-up call like create: behind whatever stream bind packed on, and done on return
        HIPCHK(hipDeviceSynchronize());
        flip_packs(v, nullptr);
        if (hipGetLastError() != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_verifier_input_grad_enable: kernel launch failed");
        HIPCHK(hipDeviceSynchronize());
    }
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_input_grad(siggan_verifier* v, const float* x, const float* ref, int32_t n, const siggan_verifier_identity* w,
                                          float* dx, float* objective, float* terms, float* score, float* emb, void* stream) {
    int rc = vcheck(v, "siggan_verifier_input_grad"); if (rc) return rc;
    if (!v->gws) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: siggan_verifier_input_grad_enable has not been called");
    if (!x || !ref || !w || !dx || !objective) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: null argument");
    const float we = w->embed_weight, ws = w->score_weight;
    if (!std::isfinite(we) || !std::isfinite(ws) || we < 0.f || ws < 0.f)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: the weights must be finite and >= 0, got (%g, %g)", (double)we, (double)ws);
    if (we == 0.f && ws == 0.f) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: both weights are 0");
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: x_dev and dx_dev must be 16-byte aligned");
    if (n < 1 || n > v->Nmax) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad: n_images %d outside [1, max_images=%d]", n, v->Nmax);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    const int E = v->E;
    float* const e = emb ? emb : v->emb;
    // forward with the decisions recorded (5), head forward + backward (1), embedding backward (1)
    if ((rc = encode<true>(v, x, x, SIGGAN_VFMT_F32, n, n, e, e, s))) return rc;
    hipLaunchKernelGGL(k_vhead_grad, dim3(n), dim3(VHID), (size_t)E * 4, s, (const float*)e, ref, n, E, (const float*)v->wc0, (const float*)v->bc0,
                       (const float*)v->wc3, (const float*)v->bc3, we, ws, v->de, objective, terms, score, v->cls_mask, v->diff_sign);
    hipLaunchKernelGGL(k_vemb_bwd, dim3(n), dim3(256), (size_t)E * 4, s, (const float*)v->de, E, (const float*)e, (const float*)v->nrm,
                       (const float*)v->wfc2, (const float*)v->fc1, v->dh, v->fc1_mask);
    // d(pool3) (n, 8192) = dh (n, 512) . Wfc1 (512, 8192), in the pack's h-w-c order (1)
    hipLaunchKernelGGL((k_tgemm<true, false>), dim3(VFC1_K / 64, (n + 63) / 64, 1), dim3(256), 0, s, (const float*)v->dh, (const float*)v->wfc1,
                       v->dp3, n, VFC1_K, VFC1_N, VFC1_N, VFC1_N, VFC1_K, VFC1_K);
    // per conv layer: un-pool (1), input gradient (1)
    int64_t total = (int64_t)n * VFC1_K;
    hipLaunchKernelGGL(k_vunpool, dim3(blocks(total)), dim3(256), 0, s, (const float*)v->dp3, (const uint8_t*)v->r3, (const float*)v->sc3, 128, 16,
                       total, v->dy3);
    hipLaunchKernelGGL((k_tconv<3, 128, 64, 16, 64>), dim3(n * 256 / 128, 1), dim3(256), 0, s, (const float*)v->dy3, (const float*)v->wf3, v->dp2);
    total = (int64_t)n * 16384;
    hipLaunchKernelGGL(k_vunpool, dim3(blocks(total)), dim3(256), 0, s, (const float*)v->dp2, (const uint8_t*)v->r2, (const float*)v->sc2, 64, 32,
                       total, v->dy2);
    hipLaunchKernelGGL((k_tconv<5, 64, 32, 32, 32>), dim3(n * 1024 / 128, 1), dim3(256), 0, s, (const float*)v->dy2, (const float*)v->wf2, v->dp1);
    total = (int64_t)n * 32768;
    hipLaunchKernelGGL(k_vunpool, dim3(blocks(total)), dim3(256), 0, s, (const float*)v->dp1, (const uint8_t*)v->r1, (const float*)v->sc1, 32, 64,
                       total, v->dy1);
    hipLaunchKernelGGL(k_vconv1_dgrad, dim3(n * 64), dim3(256), 0, s, (const float*)v->dy1, (const float*)v->w1, dx);
    v->grad_n = n;
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_input_grad: kernel launch failed");
}

extern "C" int siggan_verifier_input_grad_debug(siggan_verifier* v, const char* name, void* out, int64_t n, void* stream) {
    int rc = vcheck(v, "siggan_verifier_input_grad_debug"); if (rc) return rc;
    if (!name || !out) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad_debug: null argument");
    if (!v->gws || v->grad_n < 1) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad_debug: no input_grad call yet");
    const int64_t N = v->grad_n;
    const void* src = nullptr; int64_t total = 0; int C = 0, HW = 0;
    if (!strcmp(name, "route1")) { src = v->r1; total = N * 32768; C = 32; HW = 1024; }
    else if (!strcmp(name, "route2")) { src = v->r2; total = N * 16384; C = 64; HW = 256; }
    else if (!strcmp(name, "route3")) { src = v->r3; total = N * VFC1_K; C = 128; HW = 64; }
    else if (!strcmp(name, "fc1_mask")) { src = v->fc1_mask; total = N * VFC1_N; }
    else if (!strcmp(name, "cls_mask")) { src = v->cls_mask; total = N * VHID; }
    else if (!strcmp(name, "diff_sign")) { src = v->diff_sign; total = N * v->E; }
    else return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad_debug: unknown stage '%s'", name);
    if (n != total) return FAIL(SIGGAN_E_ARG, "siggan_verifier_input_grad_debug: '%s' holds %lld elements, caller asked for %lld", name,
                                 (long long)total, (long long)n);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    if (C) {
        hipLaunchKernelGGL(k_nchw<uint8_t>, dim3(blocks(total)), dim3(256), 0, s, (const uint8_t*)src, (uint8_t*)out, total, C, HW);
        return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_verifier_input_grad_debug: kernel launch failed");
    }
    HIPCHK(hipMemcpyAsync(out, src, (size_t)total, hipMemcpyDeviceToDevice, s));
    return SIGGAN_OK;
}

// ---------------------------------------------------------------- siggan_verifier_pairs
extern "C" int siggan_verifier_pairs_enable(siggan_verifier* v, int32_t max_queries) {
    if (!v) return FAIL(SIGGAN_E_ARG, "siggan_verifier_pairs_enable: null context");
    if (v->E > SIGGAN_PAIR_MAX_DIM)
        return FAIL(SIGGAN_E_ARG, "siggan_verifier_pairs_enable: embedding_dim %d above SIGGAN_PAIR_MAX_DIM = %d", v->E, SIGGAN_PAIR_MAX_DIM);
    if (max_queries < 1) return FAIL(SIGGAN_E_ARG, "siggan_verifier_pairs_enable: max_queries %d < 1", max_queries);
    if (v->pws && max_queries <= v->pair_max) return SIGGAN_OK;
    DevGuard dg(v->device); HIPCHK(dg.err);
    HIPCHK(hipDeviceSynchronize());                              // a set-up call: nothing may still read the workspace it replaces
    if (v->pws) { (void)hipFree(v->pws); v->pws = nullptr; v->pair_max = 0; }
    const int Kp = (v->E + PBK - 1) / PBK * PBK;
    const size_t pack = ((size_t)Kp * VHID * 4 + 255) & ~(size_t)255;
    const size_t keys = (size_t)max_queries * PSPLIT_MAX * 2 * sizeof(unsigned long long);
    char* base = nullptr;
    hipError_t e = hipMalloc((void**)&base, pack + keys);
    if (e != hipSuccess) return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", pack + keys, hipGetErrorString(e));
    v->pws = base; v->wpk = (float*)base; v->pkeys = (unsigned long long*)(base + pack);
    v->pair_kp = Kp; v->pair_max = max_queries;
    if (v->bound) {                      // behind whatever stream bind packed on (synchronised above), and done on return
        pairs_pack(v, nullptr);
        if (hipGetLastError() != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_verifier_pairs_enable: kernel launch failed");
        HIPCHK(hipDeviceSynchronize());
    }
    return SIGGAN_OK;
}

// Grid: one block column per 16 query rows; the reference tiles are split over S block rows only while the query tiles
// alone leave the device short of blocks, and never so few that a block's uint32 LDS counters could wrap (2^22 tiles of 512).
static void pair_grid(int nq, int nr, int* QT, int* S, int* tps) {
    const int ntiles = (nr + PR - 1) / PR;
    *QT = (nq + PQ - 1) / PQ;
    *S = 1;
    if (*QT < 1024) *S = std::min(std::min(PSPLIT_MAX, ntiles), (1024 + *QT - 1) / *QT);
    *S = std::max(*S, (ntiles + (1 << 22) - 1) >> 22);
    *tps = (ntiles + *S - 1) / *S;
}

extern "C" int siggan_verifier_pairs(siggan_verifier* v, const float* q, const int32_t* qid, int32_t nq, const float* r, const int32_t* rid,
                                     int32_t nr, int32_t same_set, const siggan_pair_outputs* out, void* stream) {
    const char* fn = "siggan_verifier_pairs";
    int rc = vcheck(v, fn); if (rc) return rc;
    if (v->E > SIGGAN_PAIR_MAX_DIM) return FAIL(SIGGAN_E_ARG, "%s: embedding_dim %d above SIGGAN_PAIR_MAX_DIM = %d", fn, v->E, SIGGAN_PAIR_MAX_DIM);
    if (!v->pws) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_pairs_enable has not been called", fn);
    if (!q || !r || !out) return FAIL(SIGGAN_E_ARG, "%s: null argument", fn);
    if (nq < 1 || nr < 1) return FAIL(SIGGAN_E_ARG, "%s: nq = %d, nr = %d: both must be >= 1", fn, nq, nr);
    if ((int64_t)nq * nr >= ((int64_t)1 << 62)) return FAIL(SIGGAN_E_ARG, "%s: nq * nr >= 2^62", fn);
    if (same_set && nq != nr) return FAIL(SIGGAN_E_ARG, "%s: same_set needs nq == nr, got %d and %d", fn, nq, nr);
    const int T = out->n_thresholds;
    const bool want_counts = out->threshold_dev || out->genuine_count_dev || out->impostor_count_dev || T != 0;
    const bool want_best = out->best_genuine_dev || out->best_genuine_index_dev || out->best_impostor_dev || out->best_impostor_index_dev;
    if (!out->score_dev && !want_counts && !want_best) return FAIL(SIGGAN_E_ARG, "%s: no output requested", fn);
    if (want_counts) {
        if (!out->threshold_dev || !out->genuine_count_dev || !out->impostor_count_dev)
            return FAIL(SIGGAN_E_ARG, "%s: the counts need threshold_dev, genuine_count_dev and impostor_count_dev", fn);
        if (T < 1 || T > SIGGAN_PAIR_MAX_THRESHOLDS)
            return FAIL(SIGGAN_E_ARG, "%s: n_thresholds %d outside [1, %d]", fn, T, SIGGAN_PAIR_MAX_THRESHOLDS);
    }
    if (want_best && nq > v->pair_max)
        return FAIL(SIGGAN_E_ARG, "%s: row maxima for nq = %d rows, siggan_verifier_pairs_enable was given max_queries = %d", fn, nq, v->pair_max);
    const bool vec = v->E % 4 == 0;
    auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (mis(q, vec ? 16 : 4) || mis(r, vec ? 16 : 4))
        return FAIL(SIGGAN_E_ARG, "%s: the embeddings must be %d-byte aligned", fn, vec ? 16 : 4);
    if (mis(qid, 4) || mis(rid, 4) || mis(out->score_dev, 4) || mis(out->threshold_dev, 4) || mis(out->genuine_count_dev, 8) ||
        mis(out->impostor_count_dev, 8) || mis(out->best_genuine_dev, 4) || mis(out->best_genuine_index_dev, 4) ||
        mis(out->best_impostor_dev, 4) || mis(out->best_impostor_index_dev, 4))
        return FAIL(SIGGAN_E_ARG, "%s: a pointer is not aligned to its element type", fn);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    int QT, S, tps;
    pair_grid(nq, nr, &QT, &S, &tps);
    PairOut o;
    o.list_k = o.list_flags = 0;
    o.score = out->score_dev;
    o.thr = want_counts ? out->threshold_dev : nullptr;
    o.T = want_counts ? T : 0;
    o.gcnt = (unsigned long long*)out->genuine_count_dev;
    o.icnt = (unsigned long long*)out->impostor_count_dev;
    o.keys = want_best ? v->pkeys : nullptr;
    if (want_counts) {
        HIPCHK(hipMemsetAsync(out->genuine_count_dev, 0, (size_t)(T + 1) * 8, s));
        HIPCHK(hipMemsetAsync(out->impostor_count_dev, 0, (size_t)(T + 1) * 8, s));
    }
    const size_t lds = want_counts ? ((size_t)T + 2 * ((size_t)T + 1)) * 4 : 0;
    const int upper_only = same_set && !out->score_dev && !want_best;
    auto kern = vec ? k_vpairs<true> : k_vpairs<false>;
    hipLaunchKernelGGL(kern, dim3(QT, S), dim3(256), lds, s, q, qid, (int)nq, r, rid, (int)nr, v->E, v->pair_kp, (const float*)v->wpk,
                       (const float*)v->bc0, (const float*)v->wc3, (const float*)v->bc3, (int)(same_set != 0), upper_only, tps, o);
    if (want_best)
        hipLaunchKernelGGL(k_vpairs_best, dim3(blocks(nq)), dim3(256), 0, s, (const unsigned long long*)v->pkeys, (int)nq, S,
                           out->best_genuine_dev, out->best_genuine_index_dev, out->best_impostor_dev, out->best_impostor_index_dev);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "%s: kernel launch failed", fn);
}

// ---------------------------------------------------------------- siggan_verifier_pairs_topk
extern "C" int siggan_verifier_pairs_topk_enable(siggan_verifier* v, int32_t max_queries, int32_t max_k) {
    const char* fn = "siggan_verifier_pairs_topk_enable";
    if (!v) return FAIL(SIGGAN_E_ARG, "%s: null context", fn);
    if (!v->pws) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_pairs_enable has not been called", fn);
    if (max_queries < 1) return FAIL(SIGGAN_E_ARG, "%s: max_queries %d < 1", fn, max_queries);
    if (max_k < 1 || max_k > SIGGAN_PAIR_TOPK_MAX) return FAIL(SIGGAN_E_ARG, "%s: max_k %d outside [1, %d]", fn, max_k, SIGGAN_PAIR_TOPK_MAX);
    if (v->tkeys && max_queries <= v->topk_max && max_k <= v->topk_k) return SIGGAN_OK;
    DevGuard dg(v->device); HIPCHK(dg.err);
    HIPCHK(hipDeviceSynchronize());                              // a set-up call: nothing may still read the slots it replaces
    const int rows = std::max(max_queries, v->topk_max), k = std::max(max_k, v->topk_k);      // never shrinks
    if (v->tkeys) { (void)hipFree(v->tkeys); v->tkeys = nullptr; v->topk_max = 0; v->topk_k = 0; }
    const size_t bytes = (size_t)rows * PSPLIT_MAX * 2 * k * sizeof(unsigned long long);
    hipError_t e = hipMalloc((void**)&v->tkeys, bytes);
    if (e != hipSuccess) { v->tkeys = nullptr; return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", bytes, hipGetErrorString(e)); }
    v->topk_max = rows; v->topk_k = k;
    return SIGGAN_OK;
}

extern "C" int siggan_verifier_pairs_topk(siggan_verifier* v, const float* q, const int32_t* qid, int32_t nq, const float* r,
                                          const int32_t* rid, int32_t nr, int32_t same_set, int32_t k, int32_t genuine_lowest,
                                          const siggan_pair_topk* out, void* stream) {
    const char* fn = "siggan_verifier_pairs_topk";
    int rc = vcheck(v, fn); if (rc) return rc;
    if (!v->pws) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_pairs_enable has not been called", fn);
    if (!v->tkeys) return FAIL(SIGGAN_E_ARG, "%s: siggan_verifier_pairs_topk_enable has not been called", fn);
    if (!q || !r || !out) return FAIL(SIGGAN_E_ARG, "%s: null argument", fn);
    if (nq < 1 || nr < 1) return FAIL(SIGGAN_E_ARG, "%s: nq = %d, nr = %d: both must be >= 1", fn, nq, nr);
    if ((int64_t)nq * nr >= ((int64_t)1 << 62)) return FAIL(SIGGAN_E_ARG, "%s: nq * nr >= 2^62", fn);
    if (same_set && nq != nr) return FAIL(SIGGAN_E_ARG, "%s: same_set needs nq == nr, got %d and %d", fn, nq, nr);
    if (k < 1 || k > v->topk_k) return FAIL(SIGGAN_E_ARG, "%s: k = %d outside [1, max_k = %d]", fn, k, v->topk_k);
    if (nq > v->topk_max)
        return FAIL(SIGGAN_E_ARG, "%s: nq = %d rows, siggan_verifier_pairs_topk_enable was given max_queries = %d", fn, nq, v->topk_max);
    const bool want_imp = out->impostor_score_dev || out->impostor_index_dev, want_gen = out->genuine_score_dev || out->genuine_index_dev;
    if (!want_imp && !want_gen) return FAIL(SIGGAN_E_ARG, "%s: no output requested", fn);
    const bool vec = v->E % 4 == 0;
    auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    if (mis(q, vec ? 16 : 4) || mis(r, vec ? 16 : 4))
        return FAIL(SIGGAN_E_ARG, "%s: the embeddings must be %d-byte aligned", fn, vec ? 16 : 4);
    if (mis(qid, 4) || mis(rid, 4) || mis(out->impostor_score_dev, 4) || mis(out->impostor_index_dev, 4) ||
        mis(out->genuine_score_dev, 4) || mis(out->genuine_index_dev, 4))
        return FAIL(SIGGAN_E_ARG, "%s: a pointer is not aligned to its element type", fn);
    DevGuard dg(v->device); HIPCHK(dg.err);
    hipStream_t s = (hipStream_t)stream;
    int QT, S, tps;
    pair_grid(nq, nr, &QT, &S, &tps);            // S <= PSPLIT_MAX for every int32 nr (at most 2^26 tiles): the slots hold it
    PairOut o;
    o.score = nullptr; o.thr = nullptr; o.T = 0; o.gcnt = o.icnt = nullptr;
    o.keys = v->tkeys;
    o.list_k = k;
    o.list_flags = (want_gen ? 1 : 0) | (want_imp ? 2 : 0) | (genuine_lowest ? 4 : 0);
    auto kern = vec ? k_vpairs<true, 1> : k_vpairs<false, 1>;
    hipLaunchKernelGGL(kern, dim3(QT, S), dim3(256), 0, s, q, qid, (int)nq, r, rid, (int)nr, v->E, v->pair_kp, (const float*)v->wpk,
                       (const float*)v->bc0, (const float*)v->wc3, (const float*)v->bc3, (int)(same_set != 0), 0, tps, o);
    hipLaunchKernelGGL(k_vpairs_topk_merge, dim3((2 * (int64_t)nq + 3) / 4), dim3(256), 0, s, (const unsigned long long*)v->tkeys, (int)nq,
                       S, (int)k, (int)(genuine_lowest != 0), out->genuine_score_dev, out->genuine_index_dev, out->impostor_score_dev,
                       out->impostor_index_dev);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "%s: kernel launch failed", fn);
}
