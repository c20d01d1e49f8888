// verifier_data.hip -- input pipeline of the Siamese verifier's trainer (include/siggan_verifier_data.h): gather + the
// reference's RandomAffine / RandomHorizontalFlip on cached 8-bit images, bytes in and bytes out.  gfx950 only.
//
// One launch per batch, k_pairs_augment: a thread forms four adjacent output pixels of one row and stores them as one
// aligned 32-bit word (a wave writes 256 contiguous bytes); a block of 256 threads is a quarter of one 64x64 image, so the
// image's index and its eight parameters are block-uniform.  Byte work bound by HBM / L2; no LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_verifier_data.h"
#include "host.h"

namespace {

constexpr int PS = SIGGAN_PAIRS_IMAGE_SIZE;             // 64
constexpr int PWORDS = PS * PS / 4;                     // 32-bit words per image
constexpr int PTHREADS = 256;
constexpr int PBLOCKS = PWORDS / PTHREADS;              // blocks per image
static_assert(PWORDS % PTHREADS == 0 && PS % 4 == 0, "a block must not straddle two images, a word not two rows");

__device__ __forceinline__ bool inside(int v) { return (unsigned)v < (unsigned)PS; }

// the byte of output pixel (x, y): q = this image's parameters, t = its tables (may be null)
__device__ __forceinline__ uint32_t pairs_pixel(const uint8_t* __restrict__ src, const int32_t* __restrict__ q,
                                                const int16_t* __restrict__ t, int mode, bool flip, int x, int y, uint32_t fill) {
    const int xs = flip ? PS - 1 - x : x;
    int xin, yin;
    if (mode == 0) {
        xin = xs; yin = y;
    } else if (mode == 1) {                             // Pillow's affine_fixed; unsigned so that any parameters wrap, not overflow
        xin = (int32_t)((uint32_t)q[3] + (uint32_t)y * (uint32_t)q[2] + (uint32_t)xs * (uint32_t)q[1]) >> 16;
        yin = (int32_t)((uint32_t)q[6] + (uint32_t)y * (uint32_t)q[5] + (uint32_t)xs * (uint32_t)q[4]) >> 16;
    } else {
        if (!t) return fill;
        xin = t[xs]; yin = t[PS + y];
    }
    return inside(xin) && inside(yin) ? src[yin * PS + xin] : fill;
}

__global__ __launch_bounds__(PTHREADS) void k_pairs_augment(const uint8_t* __restrict__ cache, const int32_t* __restrict__ index,
                                                            const int32_t* __restrict__ prm, const int16_t* __restrict__ tabs,
                                                            uint32_t* __restrict__ out, uint32_t fill, int64_t n_images) {
    const int b = blockIdx.x / PBLOCKS;                                   // the grid is exactly n * PBLOCKS blocks
    const int word = (blockIdx.x % PBLOCKS) * PTHREADS + threadIdx.x;    // 0..PWORDS-1 inside the image
    int64_t img = index[b];
    img = img < 0 ? 0 : (img >= n_images ? n_images - 1 : img);          // never read outside the cache
    const uint8_t* src = cache + (size_t)img * (PS * PS);
    uint32_t w;
    if (!prm) {
        w = reinterpret_cast<const uint32_t*>(src)[word];
    } else {
        const int32_t* q = prm + (size_t)b * 8;
        const int16_t* t = tabs ? tabs + (size_t)b * 2 * PS : nullptr;
        const int mode = q[0];
        const bool flip = q[7] & 1;
        const int y = word / (PS / 4), x = (word % (PS / 4)) * 4;
        w = pairs_pixel(src, q, t, mode, flip, x, y, fill) | pairs_pixel(src, q, t, mode, flip, x + 1, y, fill) << 8 |
            pairs_pixel(src, q, t, mode, flip, x + 2, y, fill) << 16 | pairs_pixel(src, q, t, mode, flip, x + 3, y, fill) << 24;
    }
    out[(size_t)b * PWORDS + word] = w;
}

}  // namespace

extern "C" int siggan_pairs_augment(int32_t device, const uint8_t* cache_dev, int64_t n_images, const int32_t* index_dev,
                                    const int32_t* params_dev, const int16_t* tables_dev, uint8_t* out_dev, int32_t n, int32_t size,
                                    int32_t fill, void* stream) {
    if (!cache_dev || !index_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: null tensor");
    if (size != PS) return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: size must be %d, got %d", PS, size);
    if (n < 1 || n > (1 << 20)) return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: n must be in 1..2^20, got %d", n);
    if (n_images < 1) return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: empty cache");
    if (fill < 0 || fill > 255) return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: fill must be a byte value");
    if ((reinterpret_cast<uintptr_t>(cache_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3)
        return FAIL(SIGGAN_E_INVALID, "siggan_pairs_augment: cache_dev and out_dev must be 4-byte aligned");
    DevGuard dg(device);
    if (dg.err != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_pairs_augment: hipSetDevice(%d) -> %s", device, hipGetErrorString(dg.err));
    hipLaunchKernelGGL(k_pairs_augment, dim3((unsigned)n * PBLOCKS), dim3(PTHREADS), 0, (hipStream_t)stream, cache_dev, index_dev,
                       params_dev, tables_dev, reinterpret_cast<uint32_t*>(out_dev), (uint32_t)fill, n_images);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_pairs_augment: kernel launch failed");
}
