// verifier_parts.h -- device parts the Siamese verifier's inference and input-gradient (verifier.hip) and training
// (verifier_train.hip) kernels are built from: the geometry, the image loads, the implicit-GEMM tile loop of conv2 / conv3, the
// raw-store conv kernel and the 64 x 64 GEMM both backward passes run, and the two halves of the fc tail.  Every sum here has
// one fixed order, and both files get the same one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "act.h"

namespace {

using siggan::f32x4;
using siggan::f32x16;

constexpr int VS = 64;                 // image size (fixed by fc1)
constexpr int VFC1_K = 8192, VFC1_N = 512, VFC1_SPLIT = 16, VFC1_KS = VFC1_K / VFC1_SPLIT;
constexpr int VHID = 64;               // classifier hidden width

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------- pair head: the expressions every kernel that scores a pair shares
// hidden unit j after bias + ReLU, from its finished dot product over |e1 - e2|
__device__ __forceinline__ float head_hidden(float dot, float b0j) { return fmaxf(dot + b0j, 0.f); }
// the similarity, from the 64 products hidden[j] * w3[j] summed in wave_sum's order
__device__ __forceinline__ float head_sigmoid(float sum, float b3) {
    const float logit = sum + b3;
    return 1.0f / (1.0f + expf(-logit));
}

// ---------------------------------------------------------------- images: fp32 as given, or bytes normalised on load
template <bool U8>
__device__ __forceinline__ float vload(const void* img, int i) {
    if (U8) {
        const float v = (float)((const uint8_t*)img)[i] / 255.0f;     // ToTensor
        return (v - 0.5f) / 0.5f;                                      // Normalize([0.5], [0.5])
    }
    return ((const float*)img)[i];
}
// image n of a batch whose first nsplit images come from x1 and the rest from x2
template <bool U8>
__device__ __forceinline__ const void* vimage(const void* x1, const void* x2, int nsplit, int n) {
    const size_t esz = U8 ? 1 : 4;
    return n < nsplit ? (const void*)((const char*)x1 + (size_t)n * VS * VS * esz)
                      : (const void*)((const char*)x2 + (size_t)(n - nsplit) * VS * VS * esz);
}

// ---------------------------------------------------------------- conv2 / conv3: the implicit-GEMM tile loop
// Which pixel (n, y, x) of the (N, H, H, .) image GEMM row m is.
// PoolRows: rows ordered (n, ph, pw, dy, dx) -- the four pixels of a pooling window are four consecutive rows aligned to 4,
// which in the 32x32 C/D layout are registers 4g..4g+3 of ONE lane.
struct PoolRows {
    static __device__ __forceinline__ void at(int64_t m, int H, int64_t& n, int& y, int& x) {
        const int HP = H / 2;
        const int64_t q = m >> 2;
        const int sub = (int)(m & 3), pw = (int)(q % HP), ph = (int)((q / HP) % HP);
        n = q / (HP * HP);
        y = 2 * ph + (sub >> 1);
        x = 2 * pw + (sub & 1);
    }
};
// RasterRows: rows in the tensor's own (n, y, x) order.
struct RasterRows {
    static __device__ __forceinline__ void at(int64_t m, int H, int64_t& n, int& y, int& x) {
        x = (int)(m % H);
        y = (int)((m / H) % H);
        n = m / (H * H);
    }
};
// acc = the 128 (M) x BN tile at (m0, n0) of the stride-1 convolution of x (N, H, H, CI) NHWC with wp [CO][KS*KS*CI].
// K-tiles of 32 (one tap, or half of one at CI = 64) staged k-major in LDS, the next tile's loads in flight under this tile's
// MFMAs; wave w owns rows [32w, 32w+32) x all BN columns (BN / 32 accumulators that share the A operand).
// C/D: acc[j][r] is row (r & 3) + 8 * (r >> 2) + 4 * lh of the wave's 32, column 32 * j + li.
// M = N * H * H is a multiple of 128, CO of BN: no ragged tiles.  Call from all 256 threads of the block.
template <int KS, int CI, int CO, int H, int BN, class Rows>
__device__ __forceinline__ void conv_tile(const float* __restrict__ x, const float* __restrict__ wp, int64_t m0, int n0,
                                          f32x16 (&acc)[BN / 32]) {
    constexpr int BM = 128, BK = 32, LDA = BM + 4, LDB = BN + 4, PAD = KS / 2, K = KS * KS * CI, NACC = BN / 32;
    constexpr int BPT = BN * BK / 256;          // B floats per thread: 8 or 4
    static_assert(CI % BK == 0 && CO % BN == 0 && (H * H) % BM == 0 && (BN == 32 || BN == 64), "tile geometry");
    __shared__ float sA[BK][LDA], sB[BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    // staging: thread -> (row, 16-float half) of A, (row, BPT floats) of B; consecutive lanes write consecutive LDS words
    const int ar = tid & 127, ah = tid >> 7;
    int64_t n;
    int y, xx;
    Rows::at(m0 + ar, H, n, y, xx);
    const float* xim = x + (size_t)n * H * H * CI + ah * 16;
    const int br = tid % BN, bq = tid / BN;
    const float* wrow = wp + (size_t)(n0 + br) * K + bq * BPT;

    f32x4 ra[4], rb[BPT / 4];
    auto fetch = [&](int k0) {
        const int tap = k0 / CI, ci0 = k0 % CI;
        const int iy = y + tap / KS - PAD, ix = xx + tap % KS - PAD;
        if (iy >= 0 && iy < H && ix >= 0 && ix < H) {                  // out-of-image taps read zeros
            const float* src = xim + ((size_t)iy * H + ix) * CI + ci0;
#pragma unroll
            for (int j = 0; j < 4; ++j) ra[j] = *reinterpret_cast<const f32x4*>(src + 4 * j);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) ra[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < BPT / 4; ++j) rb[j] = *reinterpret_cast<const f32x4*>(wrow + k0 + 4 * j);
    };
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += BK) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) sA[ah * 16 + 4 * j + e][ar] = ra[j][e];
#pragma unroll
        for (int j = 0; j < BPT / 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) sB[bq * BPT + 4 * j + e][br] = rb[j][e];
        __syncthreads();
        if (k0 + BK < K) fetch(k0 + BK);
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            const float a = sA[2 * s + lh][wave * 32 + li];
#pragma unroll
            for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, sB[2 * s + lh][32 * j + li], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- conv2 / conv3: implicit GEMM, raw store
// x: (N, H, H, CI) NHWC; wp: [CO][KS*KS*CI]; out: (N, H, H, CO).  conv_tile's 128 x BN block tile over rows in raster order.
template <int KS, int CI, int CO, int H, int BN>
__global__ __launch_bounds__(256) void k_tconv(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ out) {
    constexpr int BM = 128, NACC = BN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    f32x16 acc[NACC];
    conv_tile<KS, CI, CO, H, BN, RasterRows>(x, wp, m0, n0, acc);
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            out[(size_t)row * CO + n0 + 32 * j + li] = acc[j][r];
        }
}

// ---------------------------------------------------------------- 64 x 64 MFMA GEMM, operands K- or M/N-contiguous
// A(m, k) = AKC ? A[m * lda + k] : A[k * lda + m];  B(k, n) = BKC ? B[n * ldb + k] : B[k * ldb + n];
// C[z][m * ldc + n] over k in [z * Ks, min((z + 1) * Ks, K)).  K-contiguous operands need K % 8 == 0 and Ks % 32 == 0; the other
// kind needs its M (N) % 4 == 0.  Rows / columns / k outside the problem are staged as zeros and never stored.
template <bool AKC, bool BKC>
__global__ __launch_bounds__(256) void k_tgemm(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ Cm,
                                               int M, int N, int K, int Ks, int lda, int ldb, int ldc) {
    constexpr int BK = 32, LD = 64 + 4;
    __shared__ __attribute__((aligned(16))) float sA[BK][LD];
    __shared__ __attribute__((aligned(16))) float sB[BK][LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, lh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int n0 = blockIdx.x * 64, m0 = blockIdx.y * 64, kb = blockIdx.z * Ks, ke = min(kb + Ks, K);
    const int row = tid & 63, qd = tid >> 6;              // K-contiguous staging: (row, 8 k)
    const int c4 = (tid & 15) * 4, kk = tid >> 4;         // M-contiguous staging: (4 rows, k = kk and kk + 16)
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = kb; k0 < ke; k0 += BK) {
        if (AKC) {
            const bool ok = m0 + row < M;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + qd * 8 + 4 * j;
                const f32x4 v = (ok && k < ke) ? *reinterpret_cast<const f32x4*>(A + (size_t)(m0 + row) * lda + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) sA[qd * 8 + 4 * j + e][row] = v[e];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + kk + 16 * j;
                const f32x4 v = (k < ke && m0 + c4 < M) ? *reinterpret_cast<const f32x4*>(A + (size_t)k * lda + m0 + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(&sA[kk + 16 * j][c4]) = v;
            }
        }
        if (BKC) {
            const bool ok = n0 + row < N;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + qd * 8 + 4 * j;
                const f32x4 v = (ok && k < ke) ? *reinterpret_cast<const f32x4*>(B + (size_t)(n0 + row) * ldb + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) sB[qd * 8 + 4 * j + e][row] = v[e];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int k = k0 + kk + 16 * j;
                const f32x4 v = (k < ke && n0 + c4 < N) ? *reinterpret_cast<const f32x4*>(B + (size_t)k * ldb + n0 + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(&sB[kk + 16 * j][c4]) = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < BK / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[2 * s + lh][wm * 32 + li], sB[2 * s + lh][wn * 32 + li], acc, 0, 0, 0);
        __syncthreads();
    }
    float* cz = Cm + (size_t)blockIdx.z * M * ldc;
    const int nn = n0 + wn * 32 + li;
    if (nn < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (mm < M) cz[(size_t)mm * ldc + nn] = acc[r];
        }
    }
}

// ---------------------------------------------------------------- tail: fc1 finish, fc2, L2 norm (one 256-thread block per row)
// fc1 output j of embedding row `row`: the K slices of part [VFC1_SPLIT][M][512] summed in order, + bias, ReLU
__device__ __forceinline__ float fc1_finish(const float* __restrict__ part, int M, int row, int j, const float* __restrict__ b1) {
    float a = 0.f;
    for (int z = 0; z < VFC1_SPLIT; ++z) a += part[((size_t)z * M + row) * VFC1_N + j];
    return fmaxf(a + b1[j], 0.f);
}
// The block's hidden row sh1 [512] (LDS, just written: the barrier is taken here) -> fc2 into se [E] (LDS) and the row's
// L2 norm, clamped like F.normalize; se is complete and visible to every thread on return.
__device__ __forceinline__ float fc2_norm(const float* sh1, const float* __restrict__ w2 /* (E, 512) */,
                                          const float* __restrict__ b2, int E, float* se) {
    __shared__ float sred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();
    for (int o = wave; o < E; o += 4) {                // one wave per output: 8 products per lane, then a butterfly
        const float* wr = w2 + (size_t)o * VFC1_N;
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < VFC1_N / 64; ++i) a = fmaf(sh1[lane + 64 * i], wr[lane + 64 * i], a);
        a = wave_sum(a);
        if (lane == 0) se[o] = a + b2[o];
    }
    __syncthreads();
    float ss = 0.f;
    for (int o = tid; o < E; o += 256) ss = fmaf(se[o], se[o], ss);
    ss = wave_sum(ss);
    if (lane == 0) sred[wave] = ss;
    __syncthreads();
    return fmaxf(sqrtf((sred[0] + sred[1]) + (sred[2] + sred[3])), 1e-12f);     // F.normalize's eps
}

// ---------------------------------------------------------------- debug: NHWC -> NCHW
template <class T>
__global__ void k_nchw(const T* __restrict__ in, T* __restrict__ out, int64_t total, int C, int HW) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;     // index into out (n, c, hw)
    if (i >= total) return;
    const int hw = (int)(i % HW), c = (int)((i / HW) % C);
    const int64_t n = i / ((int64_t)HW * C);
    out[i] = in[(n * HW + hw) * C + c];
}

}  // namespace
