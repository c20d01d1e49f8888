// warp.hip -- the signature duplicator (include/siggan_warp.h): smooth random warps of byte images, bytes in and bytes out.
// gfx950 only.
//
// One launch, k_warp_u8: one 256-thread workgroup per output image.  Phase 1: the source image goes to LDS (16-byte loads
// when the image's address allows, dwords otherwise) while the first wp_groups threads draw the control points -- one Philox
// group, four control values, each -- or read them from ctrl.  Phase 2: the horizontal B-spline sums of every control row at
// every column, int32 in LDS.  Phase 3: a thread forms four adjacent pixels of one row -- the vertical sum, one rounding,
// the affine base, four byte taps from LDS -- and stores one aligned dword (a wave writes 256 contiguous bytes).  Two
// barriers, no atomics.  The ranges of every integer and the LDS layout are in warp_plan.h, checked by warp_plan_check.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_warp.h"
#include "host.h"
#include "rng.h"
#include "warp_plan.h"

static_assert(WP_MAX_SIZE == SIGGAN_WARP_MAX_SIZE && WP_PARAMS == SIGGAN_WARP_PARAMS && WP_MAX_CTRL == SIGGAN_WARP_MAX_CTRL, "header and plan");
static_assert(wp_max_amp(8) == SIGGAN_WARP_MAX_AMP(8) && wp_max_amp(16) == SIGGAN_WARP_MAX_AMP(16) && wp_max_amp(32) == SIGGAN_WARP_MAX_AMP(32),
              "header and plan");

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the source byte at (x, y), `fill` outside the image
__device__ __forceinline__ int tap(const uint8_t* img, int x, int y, int h, int w, int fill) {
    return ((unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h) ? img[y * w + x] : fill;
}

__global__ __launch_bounds__(WP_THREADS) void k_warp_u8(const uint8_t* __restrict__ src, int64_t n_src, const int32_t* __restrict__ index,
                                                        const int32_t* __restrict__ params, const int16_t* __restrict__ ctrl,
                                                        uint32_t* __restrict__ out, int32_t* __restrict__ field, int h, int w, int c,
                                                        int fill, unsigned long long seed) {
    extern __shared__ __align__(16) uint8_t lds[];
    const int l2c = wp_log2(c), gx = wp_grid(w, c), gy = wp_grid(h, c), elements = 2 * gy * gx, hw = h * w;
    const WpLayout L = wp_layout(h, w, c);
    uint8_t* img = lds + L.image;
    int32_t* D = reinterpret_cast<int32_t*>(lds + L.ctrl);
    int32_t* hs = reinterpret_cast<int32_t*>(lds + L.hsum);
    const int b = blockIdx.x, t = threadIdx.x;                          // the grid is exactly n blocks
    const int32_t* q = params + (size_t)b * WP_PARAMS;

    // ---- phase 1: the image and the control points --------------------------------------------------------------------
    int64_t s = index ? (int64_t)index[b] : (int64_t)b;
    s = s < 0 ? 0 : (s >= n_src ? n_src - 1 : s);                       // never read outside the source images
    const uint8_t* im = src + (size_t)s * hw;
    if (((reinterpret_cast<uintptr_t>(im) | (uintptr_t)hw) & 15) == 0) {
        for (int i = t; i < hw / 16; i += WP_THREADS) reinterpret_cast<uint4*>(img)[i] = reinterpret_cast<const uint4*>(im)[i];
    } else {                                                            // hw is a multiple of 4 and src 4-byte aligned
        for (int i = t; i < hw / 4; i += WP_THREADS) reinterpret_cast<uint32_t*>(img)[i] = reinterpret_cast<const uint32_t*>(im)[i];
    }
    if (t < wp_groups(h, w, c)) {
        int32_t v[4];
        if (ctrl) {
            const int16_t* cb = ctrl + (size_t)b * elements;
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * t + k;
                v[k] = e < elements ? clampi(cb[e], -WP_MAX_CTRL, WP_MAX_CTRL) : 0;
            }
        } else {
            const unsigned long long id = (unsigned long long)(uint32_t)q[0] | (unsigned long long)(uint32_t)q[1] << 32;
            const uint4 r = siggan::draw_raw(seed, id, (uint64_t)t, SIGGAN_WARP_STREAM);
            const uint32_t word[4] = {r.x, r.y, r.z, r.w};
            const int amp[2] = {clampi(q[2], 0, wp_max_amp(c)), clampi(q[3], 0, wp_max_amp(c))};
            for (int k = 0; k < 4; ++k) {
                const int e = 4 * t + k;
                const int sv = (int32_t)(word[k] >> 16) - 32768;
                v[k] = (sv * amp[e >= gy * gx ? 1 : 0]) >> 15;           // elements past the grid are never read
            }
        }
        for (int k = 0; k < 4; ++k) D[4 * t + k] = v[k];                // whole groups: the region holds 4 * groups ints
    }
    __syncthreads();

    // ---- phase 2: hs[comp][j][x] = sum_a B_a(x mod c) D[comp][j][x / c + a] --------------------------------------------
    for (int i = t; i < 2 * gy * w; i += WP_THREADS) {
        const int x = i % w, row = i / w;                               // row = comp * gy + j
        const int k = x & (c - 1);
        const int32_t* d = D + row * gx + (x >> l2c);
        hs[i] = wp_weight(0, k, c) * d[0] + wp_weight(1, k, c) * d[1] + wp_weight(2, k, c) * d[2] + wp_weight(3, k, c) * d[3];
    }
    __syncthreads();

    // ---- phase 3: four adjacent pixels per thread ----------------------------------------------------------------------
    const int wq = w >> 2;
    const int64_t a0 = q[4], a1 = q[5], a2 = q[6], a3 = q[7], a4 = q[8], a5 = q[9];
    for (int word = t; word < hw / 4; word += WP_THREADS) {
        const int y = word / wq, x4 = (word - y * wq) * 4;
        const int ky = y & (c - 1);
        const int64_t w0 = wp_weight(0, ky, c), w1 = wp_weight(1, ky, c), w2 = wp_weight(2, ky, c), w3 = wp_weight(3, ky, c);
        const int32_t* hx = hs + (y >> l2c) * w;                        // control rows cy .. cy + 3 of the x plane
        const int32_t* hy = hx + gy * w;
        uint32_t packed = 0;
        for (int k = 0; k < 4; ++k) {
            const int x = x4 + k;
            const int dx = wp_round(w0 * hx[x] + w1 * hx[w + x] + w2 * hx[2 * w + x] + w3 * hx[3 * w + x], l2c);
            const int dy = wp_round(w0 * hy[x] + w1 * hy[w + x] + w2 * hy[2 * w + x] + w3 * hy[3 * w + x], l2c);
            if (field) {
                field[((size_t)b * 2) * hw + y * w + x] = dx;
                field[((size_t)b * 2 + 1) * hw + y * w + x] = dy;
            }
            // the base in 64 bits, so no parameter row wraps; a position two pixels or more outside reads `fill` at all
            // four taps whatever its fraction, so it may be clamped there and the rest is 32-bit
            int64_t bx = ((a2 + y * a1 + x * a0) >> 8) + dx, by = ((a5 + y * a4 + x * a3) >> 8) + dy;
            bx = bx < -512 ? -512 : (bx > (int64_t)(w + 1) * 256 ? (int64_t)(w + 1) * 256 : bx);
            by = by < -512 ? -512 : (by > (int64_t)(h + 1) * 256 ? (int64_t)(h + 1) * 256 : by);
            const int px = (int)bx, py = (int)by;
            const int x0 = px >> 8, fx = px & 255, y0 = py >> 8, fy = py & 255;
            const int p00 = tap(img, x0, y0, h, w, fill), p10 = tap(img, x0 + 1, y0, h, w, fill);
            const int p01 = tap(img, x0, y0 + 1, h, w, fill), p11 = tap(img, x0 + 1, y0 + 1, h, w, fill);
            const int v = ((256 - fx) * (256 - fy) * p00 + fx * (256 - fy) * p10 + (256 - fx) * fy * p01 + fx * fy * p11 + 32768) >> 16;
            packed |= (uint32_t)v << (8 * k);
        }
        out[(size_t)b * (hw / 4) + word] = packed;
    }
}

}  // namespace

extern "C" int siggan_warp_u8(int32_t device, const uint8_t* src_dev, int64_t n_src, const int32_t* index_dev, const int32_t* params_dev,
                              const int16_t* ctrl_dev, uint8_t* out_dev, int32_t* field_dev, int32_t n, int32_t h, int32_t w, int32_t cell,
                              int32_t fill, uint64_t seed, void* stream) {
    if (!src_dev || !params_dev || !out_dev) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: null tensor");
    if (n < 1 || n > WP_MAX_N) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: n must be in 1..2^20, got %d", n);
    if (n_src < 1) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: no source image");
    if (h < 1 || h > WP_MAX_SIZE) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: h must be in 1..%d, got %d", WP_MAX_SIZE, h);
    if (w < 4 || w > WP_MAX_SIZE || w % 4) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: w must be a multiple of 4 in 4..%d, got %d", WP_MAX_SIZE, w);
    if (!wp_cell_ok(cell)) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: cell must be 8, 16 or 32, got %d", cell);
    if (fill < 0 || fill > 255) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: fill must be a byte value");
    if ((reinterpret_cast<uintptr_t>(src_dev) | reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(field_dev) |
         reinterpret_cast<uintptr_t>(params_dev) | reinterpret_cast<uintptr_t>(index_dev)) & 3)
        return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: src_dev, out_dev, field_dev, params_dev and index_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(ctrl_dev) & 1) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: ctrl_dev must be 2-byte aligned");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src_dev), o0 = reinterpret_cast<uintptr_t>(out_dev);
    if (o0 < s0 + (uintptr_t)n_src * h * w && s0 < o0 + (uintptr_t)n * h * w) return FAIL(SIGGAN_E_INVALID, "siggan_warp_u8: out_dev overlaps src_dev");
    DevGuard dg(device);
    if (dg.err != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_warp_u8: hipSetDevice(%d) -> %s", device, hipGetErrorString(dg.err));
    hipLaunchKernelGGL(k_warp_u8, dim3((unsigned)n), dim3(WP_THREADS), (size_t)wp_layout(h, w, cell).bytes, (hipStream_t)stream, src_dev, n_src,
                       index_dev, params_dev, ctrl_dev, reinterpret_cast<uint32_t*>(out_dev), field_dev, h, w, cell, fill,
                       (unsigned long long)seed);
    return hipGetLastError() == hipSuccess ? SIGGAN_OK : FAIL(SIGGAN_E_HIP, "siggan_warp_u8: kernel launch failed");
}
