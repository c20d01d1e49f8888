// paramgrad.hip -- the kernels of siggan_g_param_grad that neither the training step nor the latent calls already have
// (gfx950, fp32 tensors): the eval-mode BatchNorm parameter sums of a Generator block with dy = scale * dpost, the final conv's
// weight / bias gradient from the stored last activation, and the fc block's BatchNorm1d sums.
//
// BatchNorm here is the fixed per-channel affine it is in eval mode: dbeta[c] = sum dpost, dgamma[c] = sum dpost * xhat with
// xhat = (y - running_mean) * rstd taken from the PRE-BatchNorm tensor y, never from the stored activation -- so dgamma is
// right for gamma of either sign and for gamma == 0 -- and dy = scale * dpost, none of the training backward's batch terms.
//
// Every sum has a fixed order (index order inside a thread, lane order in LDS, chunk order in k_part_sum) and nothing is
// accumulated with atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include "ops.h"

namespace siggan {

typedef f32x4 f4v;
__device__ __forceinline__ f4v ldg4(const float* p) { return *reinterpret_cast<const f4v*>(p); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// =========================================================================================
// the second stage of every reduction here: out[e] = sum over chunks of part[chunk][e], E entries per chunk.  A workgroup owns
// 32 consecutive entries (one coalesced 128-byte read per chunk); lane k of 32 adds chunks k, k + 32, ... in index order, the
// 32 lanes meet in LDS in lane order.  Where entry e goes: BN -- [dbeta | dgamma] of `split` channels each; TAPS -- the final
// conv's weight, entry tap * 32 + c -> torch's c * 9 + tap, and entry 288 its bias.
// =========================================================================================
enum PartOut : int { PO_BN = 0, PO_TAPS = 1 };
__global__ __launch_bounds__(1024) void k_part_sum(const float* __restrict__ part, int nch, int E, int mode, int split,
                                                   float* __restrict__ o0, float* __restrict__ o1) {
    __shared__ float sh[32][33];
    const int j = threadIdx.x & 31, k = threadIdx.x >> 5, e = blockIdx.x * 32 + j;
    float s = 0.f;
    if (e < E)
        for (int ch = k; ch < nch; ch += 32) s += part[(size_t)ch * E + e];
    sh[k][j] = s;
    __syncthreads();
    if (threadIdx.x < 32 && e < E) {
        float t = sh[0][j];
        for (int q = 1; q < 32; ++q) t += sh[q][j];
        if (mode == PO_BN) { if (e < split) o0[e] = t; else o1[e - split] = t; }
        else { if (e < 288) o0[(e & 31) * 9 + (e >> 5)] = t; else o1[0] = t; }
    }
}

// =========================================================================================
// eval-mode BatchNorm backward of one block: g [R][C] holds dpost = d(activation output) * act' (the input-gradient GEMM's
// EPI_LRELU_BWD epilogue, or k_final_dgrad_eval, applied the mask) and leaves as dy = scale[c] * dpost; y [R][C] is the block's
// pre-BatchNorm output.  256 threads = C / 4 channel lanes (a float4 each) x 1024 / C row lanes; a workgroup walks `rows`
// consecutive rows and writes ONE partial row [sum dpost | sum dpost * xhat] of 2 C floats.
// =========================================================================================
__global__ __launch_bounds__(256) void k_bn_eval_bwd(float* g, const float* __restrict__ y, int64_t R, int C, int rows,
                                                     const float* __restrict__ bne, float* __restrict__ part) {
    __shared__ f4v sh[2][256];
    const int C4 = C >> 2, c4 = threadIdx.x % C4, rl = threadIdx.x / C4, RP = 256 / C4;
    const f4v sc = ldg4(bne + c4 * 4), mean = ldg4(bne + 2 * C + c4 * 4), rstd = ldg4(bne + 3 * C + c4 * 4);
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = r0 + rows < R ? r0 + rows : R;
    f4v sb = {0.f, 0.f, 0.f, 0.f}, sg = {0.f, 0.f, 0.f, 0.f};
    for (int64_t r = r0 + rl; r < r1; r += RP) {
        const size_t i = (size_t)r * C + c4 * 4;
        const f4v d = ldg4(g + i), v = ldg4(y + i);
        f4v o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (v[e] - mean[e]) * rstd[e];
            sb[e] += d[e];
            sg[e] = fmaf(d[e], xh, sg[e]);
            o[e] = d[e] * sc[e];
        }
        *reinterpret_cast<f4v*>(g + i) = o;
    }
    sh[0][threadIdx.x] = sb; sh[1][threadIdx.x] = sg;
    __syncthreads();
    if (threadIdx.x < 2 * C4) {
        const int stat = threadIdx.x / C4, cc = threadIdx.x % C4;
        f4v t = sh[stat][cc];
        for (int q = 1; q < RP; ++q) { const f4v u = sh[stat][q * C4 + cc]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        *reinterpret_cast<f4v*>(part + ((size_t)blockIdx.x * 2 + stat) * C + cc * 4) = t;
    }
}

bool launch_bn_eval_bwd(float* g, const float* y, int64_t R, int C, const float* bne, float* part, int64_t part_cap,
                        float* dgamma, float* dbeta, hipStream_t s) {
    if (C < 32 || C > 512 || (C & (C - 1)) != 0) return false;        // (the blocks' channel counts: 32 .. 256; 2 * C / 4 <= 256 threads combine)
    int64_t rows = 512;                                                // (restated in tests/evalpaths.py)
    while (cdiv(R, rows) * 2 * (int64_t)C > part_cap) rows *= 2;
    const int nch = cdiv(R, rows);
    hipLaunchKernelGGL(k_bn_eval_bwd, dim3((unsigned)nch), dim3(256), 0, s, g, y, R, C, (int)rows, bne, part);
    hipLaunchKernelGGL(k_part_sum, dim3((unsigned)cdiv(2 * C, 32)), dim3(1024), 0, s, (const float*)part, nch, 2 * C, (int)PO_BN, C,
                       dbeta, dgamma);
    return true;
}

// =========================================================================================
// final 3x3 conv (32 -> 1): dW[c][kh][kw] = sum_{n,y,x} dpre[n][y + 1 - kh][x + 1 - kw] * a[n][y][x][c], db = sum dpre, from
// the stored last activation a.  The strip layout of k_final_dgrad_eval: 8 lanes per pixel (4 channels each) x 32 pixels along
// a row; a workgroup owns `rows` rows (a multiple of 8) of a 32-pixel column band of one image, walks them 8 at a time with the
// (8 + 2) x 34 dpre neighbourhood (zero outside the image) in LDS, and every element of a is read exactly once.  The 32 pixel
// lanes then meet in LDS in lane order: one partial row of 288 + 1 floats per workgroup.
// =========================================================================================
__global__ __launch_bounds__(256) void k_final_wgrad_eval(const float* __restrict__ dpre, const float* __restrict__ a,
                                                          float* __restrict__ part, int S, int rows) {
    constexpr int RY = 8, C = 32, PW = 34;
    __shared__ float sp[(RY + 2) * PW];
    __shared__ float sacc[32][8 * 36 + 1];
    __shared__ float sbias[32];
    const int c4 = threadIdx.x & 7, xi = threadIdx.x >> 3;
    const int nbx = S >> 5, nby = S / rows;
    int sid = blockIdx.x;
    const int xb = (sid % nbx) * 32; sid /= nbx;
    const int y0 = (sid % nby) * rows, n = sid / nby;
    f4v acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = f4v{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int ys = y0; ys < y0 + rows; ys += RY) {
        __syncthreads();                                   // the previous strip's neighbourhood has been read
        for (int e = threadIdx.x; e < (RY + 2) * PW; e += 256) {
            const int r = e / PW, k = e - r * PW;
            const int yy = ys + r - 1, xx = xb + k - 1, yc = clampi(yy, S - 1), xc = clampi(xx, S - 1);
            const float q = dpre[((size_t)n * S + yc) * S + xc];
            sp[e] = (yy == yc && xx == xc) ? q : 0.f;
        }
        __syncthreads();
        const size_t o0 = (((size_t)n * S + ys) * S + xb + xi) * C + c4 * 4;
#pragma unroll
        for (int r = 0; r < RY; ++r) {
            const f4v v = ldg4(a + o0 + (size_t)r * S * C);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float d = sp[(r + 2 - kh) * PW + xi + 2 - kw];       // dpre[y + 1 - kh][x + 1 - kw]
                    f4v& t = acc[kh * 3 + kw];
                    t.x = fmaf(d, v.x, t.x); t.y = fmaf(d, v.y, t.y); t.z = fmaf(d, v.z, t.z); t.w = fmaf(d, v.w, t.w);
                }
            if (c4 == 0) bsum += sp[(r + 1) * PW + xi + 1];                   // the pixel's own dpre
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float* const q = &sacc[xi][c4 * 36 + k * 4];
        q[0] = acc[k].x; q[1] = acc[k].y; q[2] = acc[k].z; q[3] = acc[k].w;
    }
    if (c4 == 0) sbias[xi] = bsum;
    __syncthreads();
    float* const out = part + (size_t)blockIdx.x * 289;
    for (int e = threadIdx.x; e < 289; e += 256) {
        float t;
        if (e < 288) {
            const int k = e >> 5, c = e & 31, col = (c >> 2) * 36 + k * 4 + (c & 3);
            t = sacc[0][col];
            for (int q = 1; q < 32; ++q) t += sacc[q][col];
        } else {
            t = sbias[0];
            for (int q = 1; q < 32; ++q) t += sbias[q];
        }
        out[e] = t;
    }
}

bool launch_final_wgrad_eval(const float* dpre, const float* a, float* part, int64_t part_cap, float* dW, float* db, int B, int S,
                             hipStream_t s) {
    int rows = 8;
    while (rows < S && (int64_t)B * (S / 32) * (S / rows) * 289 > part_cap) rows *= 2;
    const int64_t nblk = (int64_t)B * (S / 32) * (S / rows);
    if (nblk * 289 > part_cap || S % 32 != 0) return false;
    hipLaunchKernelGGL(k_final_wgrad_eval, dim3((unsigned)nblk), dim3(256), 0, s, dpre, a, part, S, rows);
    hipLaunchKernelGGL(k_part_sum, dim3((unsigned)cdiv(289, 32)), dim3(1024), 0, s, (const float*)part, (int)nblk, 289, (int)PO_TAPS, 0,
                       dW, db);
    return true;
}

// =========================================================================================
// the fc block's BatchNorm1d in eval form.  One wave per feature f' (NHWC order, f = c * 16 + hw in torch's): the folded
// forward kept only the activation a0, so the pre-BatchNorm value y[b] = z[b,:] . W[f,:] + bias[f] is formed again here (lane =
// latent index, index order per lane, then the butterfly: every lane holds the same sum), xhat from it and the running
// statistics.  dpost = g_dact(a0) * dh;  dbeta[f] = sum_b dpost, dgamma[f] = sum_b dpost * xhat (batch order), and dh leaves as
// scale0[f'] * dpost -- what launch_fc_wgrad turns into the Linear's dW and db.  Any K >= 1, any B >= 1.
// =========================================================================================
template <bool LK>
__global__ __launch_bounds__(256) void k_fc_bn_eval_bwd(float* dh, const float* __restrict__ a0, const float* __restrict__ bne,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        const float* __restrict__ z, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, int B, int K, int C0, int F, float gs) {
    const int lane = threadIdx.x & 63, fp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (fp >= F) return;                                   // (a whole wave)
    const int f = (fp % C0) * 16 + fp / C0;
    const float sc = bne[fp], mean = bne[2 * F + fp], rstd = bne[3 * F + fp], bf = bias[f];
    const float* const w = W + (size_t)f * K;
    float sb = 0.f, sg = 0.f;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s = fmaf(w[k], z[(size_t)b * K + k], s);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
        const float xh = ((s + bf) - mean) * rstd;
        const size_t idx = (size_t)b * F + fp;
        const float d = g_dact<LK>(a0[idx], dh[idx], gs);
        sb += d;
        sg = fmaf(d, xh, sg);
        if (lane == 0) dh[idx] = d * sc;
    }
    if (lane == 0) { dbeta[f] = sb; dgamma[f] = sg; }
}

void launch_fc_bn_eval_bwd(float* dh, const float* a0, const float* bne, const float* W, const float* bias, const float* z,
                           float* dgamma, float* dbeta, int B, int K, int C0, float gslope, hipStream_t s) {
    const int F = C0 * 16;
    SIGGAN_GS_SWITCH(gslope, LK, hipLaunchKernelGGL((k_fc_bn_eval_bwd<LK>), dim3((unsigned)cdiv(F, 4)), dim3(256), 0, s, dh, a0, bne, W,
                                                    bias, z, dgamma, dbeta, B, K, C0, F, gslope));
}

}  // namespace siggan
