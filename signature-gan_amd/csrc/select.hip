// select.hip -- ranking and gathering on the device (include/siggan_select.h): the tail of realism-filtered generation.
// gfx950 only.
//
// k_select_rank: thread i owns score i and counts the scores that come before it in the order "higher first, equal scores
// by ascending index"; the scores pass through LDS a tile at a time as ORDER KEYS -- the bit pattern mapped to a signed
// integer that sorts like the float, -0.0 folded onto 0.0 -- so every comparison is an integer one and a subnormal score
// is ordered by its value whatever the float mode.  All lanes of a wave read the same LDS word (a broadcast), four keys
// per read.  The ranks are a permutation of [0, m): each index[rank] has exactly one writer.
// k_gather_u8: block (chunk, r) copies 256 words of image index[r] to row r, binarising the four bytes of a word when asked.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/siggan_select.h"
#include "host.h"

namespace {

constexpr int TILE = 2048;                               // keys per LDS tile (8 KiB)

__device__ __forceinline__ int order_key(float s) {
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0u;                                        // -0.0 == 0.0
    return (int)(u ^ ((unsigned)((int)u >> 31) & 0x7fffffffu));          // negative floats: larger magnitude, smaller key
}
__device__ __forceinline__ int before(int kj, int ki, int j, int i) { return (kj > ki) | ((kj == ki) & (j < i)); }

__global__ __launch_bounds__(256) void k_select_rank(const float* __restrict__ scores, int m, int k, int32_t* __restrict__ index) {
    __shared__ __attribute__((aligned(16))) int sk[TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int ki = i < m ? order_key(scores[i]) : 0;
    int rank = 0;
    for (int j0 = 0; j0 < m; j0 += TILE) {
        const int n = min(TILE, m - j0), n4 = (n + 3) & ~3;
        __syncthreads();                                                 // the previous tile has been read by every wave
        // the tail of the last quad holds INT_MIN at positions j >= m > i: neither test of before() can pass there
        for (int t = threadIdx.x; t < n4; t += 256) sk[t] = t < n ? order_key(scores[j0 + t]) : INT_MIN;
        __syncthreads();
        if (i < m)
            for (int t = 0; t < n4; t += 4) {
                const int4 q = *reinterpret_cast<const int4*>(sk + t);
                const int j = j0 + t;
                rank += before(q.x, ki, j, i) + before(q.y, ki, j + 1, i) + before(q.z, ki, j + 2, i) + before(q.w, ki, j + 3, i);
            }
    }
    if (i < m && rank < k) index[rank] = i;
}

__device__ __forceinline__ unsigned binarize_word(unsigned w, int thr) {
    unsigned o = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) o |= ((int)((w >> (8 * b)) & 255u) < thr ? 0u : 255u) << (8 * b);
    return o;
}
__global__ __launch_bounds__(256) void k_gather_u8(const unsigned* __restrict__ pool, int m, int words, int chunks,
                                                   const int32_t* __restrict__ index, int binarize, unsigned* __restrict__ out) {
    const int r = blockIdx.x / chunks, w = (blockIdx.x % chunks) * 256 + threadIdx.x;
    const int src = index[r];
    if (w >= words || (unsigned)src >= (unsigned)m) return;
    unsigned v = pool[(size_t)src * words + w];
    if (binarize >= 0) v = binarize_word(v, binarize);
    out[(size_t)r * words + w] = v;
}

}  // namespace

extern "C" int siggan_select_topk(int32_t device, const float* scores_dev, int32_t m, int32_t k, int32_t* index_dev, void* stream) {
    if (!scores_dev || !index_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (m < 1 || m > SIGGAN_SELECT_MAX) return FAIL(SIGGAN_E_INVALID, "m = %d outside [1, %d]", m, SIGGAN_SELECT_MAX);
    if (k < 1 || k > m) return FAIL(SIGGAN_E_INVALID, "k = %d outside [1, m = %d]", k, m);
    DevGuard dg(device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_select_rank, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, (hipStream_t)stream, scores_dev, m, k, index_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

extern "C" int siggan_gather_u8(int32_t device, const uint8_t* pool_dev, int32_t m, int64_t pixels, const int32_t* index_dev,
                                int32_t k, int32_t binarize, uint8_t* out_dev, void* stream) {
    if (!pool_dev || !index_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (m < 1 || k < 1) return FAIL(SIGGAN_E_INVALID, "bad pool size m = %d / selection size k = %d", m, k);
    if (pixels < 4 || (pixels & 3)) return FAIL(SIGGAN_E_INVALID, "pixels must be a positive multiple of 4, got %lld", (long long)pixels);
    if (binarize < -1 || binarize > 255) return FAIL(SIGGAN_E_INVALID, "binarize must be -1 (off) or a byte value, got %d", binarize);
    if ((reinterpret_cast<uintptr_t>(pool_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3)
        return FAIL(SIGGAN_E_INVALID, "pool_dev and out_dev must be 4-byte aligned");
    const int64_t words = pixels >> 2, chunks = (words + 255) / 256;
    if (words > INT32_MAX || (int64_t)k * chunks > INT32_MAX) return FAIL(SIGGAN_E_INVALID, "selection too large for one launch");
    DevGuard dg(device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_gather_u8, dim3((unsigned)((int64_t)k * chunks)), dim3(256), 0, (hipStream_t)stream, (const unsigned*)pool_dev, m,
                       (int)words, (int)chunks, index_dev, binarize, (unsigned*)out_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
