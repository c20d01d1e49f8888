// ssim.hip -- single-scale SSIM between byte images (include/siggan_ssim.h).  gfx950 only.
//
// filter_rows: the one device function that applies the separable 11-tap window to a stream of rows.  A wave owns an image
// (or a pair of images); a lane owns column `lane` (and `lane + 64` beyond 64 columns).  Row r of the stream -- x, x x or
// x y, whatever the source gives -- goes into one of the wave's two LDS rows, every lane forms the horizontal sum of its
// column from eleven neighbours (fmaf chain, taps ascending) and pushes it into the vertical filter, which is kept in
// transposed form: ten running sums per column, v[k] = fmaf(g[k], hrow, v[k - 1]), so each horizontal value is formed once,
// the sum of an output row receives its taps in ascending order as the rows arrive, and nothing is shifted or indexed
// dynamically.  From row 10 on every row completes output row r - 10, which the sink takes.
//
// k_ssim_prepare: one wave per image; two passes of filter_rows, over x (-> mu) and over x x (-> var = G * (x x) - mu mu).
// k_ssim_pairs:   a workgroup of up to four waves keeps one a-image per wave as bytes in LDS and walks its slice of the
//   columns in chunks of b-images staged as bytes in LDS for all its waves.  Per pair only G * (x y) is filtered; the sink
//   reads the two images' prepared map rows, forms s with one division and keeps one partial sum per lane, which a fixed
//   butterfly in the wave ends.  The splits of the columns and a row's `best` as a key (HighestF32) are image_pairs.h's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/siggan_ssim.h"
#include "image_pairs.h"
#include "ink_rows.h"

namespace {

constexpr int TAPS = SIGGAN_SSIM_TAPS;
constexpr int HALO = TAPS - 1;
constexpr int STAGE_BYTES = 16384;       // of b-images per chunk
constexpr int MAX_CHUNK = 8;             // b-images per chunk at most
constexpr float SSIM_C1 = (float)((0.01 * 255.0) * (0.01 * 255.0));
constexpr float SSIM_C2 = (float)((0.03 * 255.0) * (0.03 * 255.0));

struct Taps { float g[TAPS]; };

Taps host_taps() {
    double e[TAPS], sum = 0.0;
    for (int k = 0; k < TAPS; ++k) {
        const double d = (double)(k - TAPS / 2);
        e[k] = exp(-(d * d) / (2.0 * SIGGAN_SSIM_SIGMA * SIGGAN_SSIM_SIGMA));
        sum += e[k];
    }
    Taps t;
    for (int k = 0; k < TAPS; ++k) t.g[k] = (float)(e[k] / sum);
    return t;
}

// The lanes of one wave have written LDS that other lanes of the same wave are about to read.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// rows: the wave's 2 * w floats of LDS.  src(r, c): element (r, c) of the stream, 0 <= c < w.  sink.load(o, c, q) is called
// before the LDS work of the row that completes output row o (a place to start global loads), sink.take(o, c, q, value)
// after it; q numbers the lane's columns, c = lane + 64 q < w - 10.  All 64 lanes of the wave must call this together.
template <int NC, typename Src, typename Sink>
__device__ __forceinline__ void filter_rows(const Taps& t, float* rows, int h, int w, int lane, Src src, Sink& sink) {
    const int ow = w - HALO;
    float v[NC][HALO];
#pragma unroll
    for (int q = 0; q < NC; ++q)
#pragma unroll
        for (int k = 0; k < HALO; ++k) v[q][k] = 0.0f;
    for (int r = 0; r < h; ++r) {
        float* row = rows + (r & 1) * w;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int c = lane + 64 * q;
            if (c < w) row[c] = src(r, c);
        }
        if (r >= HALO) {
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if (lane + 64 * q < ow) sink.load(r - HALO, lane + 64 * q, q);
        }
        wave_sync();
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const int c = lane + 64 * q;
            if (c < ow) {
                float hv = t.g[0] * row[c];
#pragma unroll
                for (int k = 1; k < TAPS; ++k) hv = fmaf(t.g[k], row[c + k], hv);
                const float out = fmaf(t.g[HALO], hv, v[q][HALO - 1]);
#pragma unroll
                for (int k = HALO - 1; k > 0; --k) v[q][k] = fmaf(t.g[k], hv, v[q][k - 1]);
                v[q][0] = t.g[0] * hv;
                if (r >= HALO) sink.take(r - HALO, c, q, out);
            }
        }
    }
}

struct StoreSink {                        // plane 0: mu
    float* out; int ow;
    __device__ __forceinline__ void load(int, int, int) {}
    __device__ __forceinline__ void take(int o, int c, int, float value) { out[o * ow + c] = value; }
};
template <int NC> struct VarSink {        // plane 1: G * (x x) - mu mu, mu read back from plane 0 (this lane wrote it)
    const float* mu; float* out; int ow; float m[NC];
    __device__ __forceinline__ void load(int o, int c, int q) { m[q] = mu[o * ow + c]; }
    __device__ __forceinline__ void take(int o, int c, int q, float value) { out[o * ow + c] = value - m[q] * m[q]; }
};

template <int NC>
__global__ __launch_bounds__(256) void k_ssim_prepare(Taps t, const uint8_t* __restrict__ u8, int n, int h, int w, float* maps) {
    __shared__ float srow[4][2 * SIGGAN_SSIM_MAX_SIZE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int img = blockIdx.x * 4 + wave;
    if (img >= n) return;                                                // wave-uniform; nothing below synchronises waves
    const int oh = h - HALO, ow = w - HALO;
    const uint8_t* x = u8 + (size_t)img * h * w;
    float* mu = maps + (size_t)img * 2 * oh * ow;
    float* var = mu + (size_t)oh * ow;
    StoreSink s0{mu, ow};
    filter_rows<NC>(t, srow[wave], h, w, lane, [&](int r, int c) { return (float)x[r * w + c]; }, s0);
    wave_sync();                                                         // the last row's readers before the next pass writes
    VarSink<NC> s1{mu, var, ow, {}};
    filter_rows<NC>(t, srow[wave], h, w, lane, [&](int r, int c) { const float f = (float)x[r * w + c]; return f * f; }, s1);
}

template <int NC> struct PairSink {
    const float* amu; const float* avar; const float* bmu; const float* bvar; int ow;
    float mx[NC], vx[NC], my[NC], vy[NC], sum;
    __device__ __forceinline__ void load(int o, int c, int q) {
        const int e = o * ow + c;
        mx[q] = amu[e]; vx[q] = avar[e]; my[q] = bmu[e]; vy[q] = bvar[e];
    }
    __device__ __forceinline__ void take(int, int, int q, float gxy) {
        const float mxy = mx[q] * my[q];
        const float cov = gxy - mxy;
        const float num = (2.0f * mxy + SSIM_C1) * (2.0f * cov + SSIM_C2);
        const float den = (mx[q] * mx[q] + my[q] * my[q] + SSIM_C1) * (vx[q] + vy[q] + SSIM_C2);
        sum += num / den;
    }
};

// grid (ceil(na / RW), splits), RW = blockDim.x / 64 waves = a-images per workgroup.  Dynamic LDS: RW * 2 * w floats, then
// RW a-images, then `chunk` b-images, h * w bytes each.  In PAIRED mode a workgroup's columns are its own rows.
template <int NC>
__global__ __launch_bounds__(256) void k_ssim_pairs(Taps t, const uint8_t* __restrict__ a_u8, const float* __restrict__ a_maps, int na,
                                                    const uint8_t* __restrict__ b_u8, const float* __restrict__ b_maps, int nb, int h,
                                                    int w, int mode, int chunk, int per, float* __restrict__ matrix,
                                                    unsigned long long* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, RW = blockDim.x >> 6, threads = blockDim.x;
    const int hw = h * w, words = hw >> 2, oh = h - HALO, ow = w - HALO;
    const size_t plane = (size_t)oh * ow;
    float* rows = reinterpret_cast<float*>(smem) + wave * 2 * w;
    unsigned* sa32 = reinterpret_cast<unsigned*>(smem + (size_t)RW * 2 * w * sizeof(float));
    unsigned* sb32 = sa32 + RW * words;
    const uint8_t* sa = reinterpret_cast<const uint8_t*>(sa32) + wave * hw;
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(sb32);
    const int split = blockIdx.y, S = gridDim.y, i0 = blockIdx.x * RW, i = i0 + wave;
    const bool paired = mode == SIGGAN_SSIM_PAIRED, same = mode == SIGGAN_SSIM_SAME_SET;
    const int j_begin = paired ? i0 : split * per;
    const int j_end = paired ? min(i0 + RW, nb) : min(nb, j_begin + per);

    const int na_here = min(RW, na - i0);                               // >= 1
    for (int e = tid; e < na_here * words; e += threads)
        sa32[e] = reinterpret_cast<const unsigned*>(a_u8 + (size_t)i0 * hw)[e];
    const float count = (float)(oh * ow);
    unsigned long long best = HighestF32::NONE;
    for (int jc = j_begin; jc < j_end; jc += chunk) {
        const int cnt = min(chunk, j_end - jc);
        __syncthreads();                                                 // the previous chunk is consumed
        for (int e = tid; e < cnt * words; e += threads)
            sb32[e] = reinterpret_cast<const unsigned*>(b_u8 + (size_t)jc * hw)[e];
        __syncthreads();
        if (i >= na) continue;                                           // wave-uniform; the barriers above are still reached
        for (int jj = 0; jj < cnt; ++jj) {
            const int j = jc + jj;
            if (paired && j != i) continue;
            if (same && j == i && !matrix) continue;
            const uint8_t* y = sb + jj * hw;
            PairSink<NC> sink{a_maps + (size_t)i * 2 * plane, a_maps + (size_t)i * 2 * plane + plane,
                              b_maps + (size_t)j * 2 * plane, b_maps + (size_t)j * 2 * plane + plane, ow, {}, {}, {}, {}, 0.0f};
            filter_rows<NC>(t, rows, h, w, lane, [&](int r, int c) { return (float)sa[r * w + c] * (float)y[r * w + c]; }, sink);
            float total = sink.sum;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
            const float value = total / count;
            if (matrix && lane == 0) matrix[matrix_slot(paired, i, j, nb)] = value;
            if (!(same && j == i)) keep_better<HighestF32>(best, value, j);
            wave_sync();                                                 // the last row's readers before the next pair writes
        }
    }
    if (keys && i < na && lane == 0) keys[(size_t)i * S + split] = best;
}

int check_size(int32_t h, int32_t w) {
    if (h < SIGGAN_SSIM_MIN_HEIGHT || h > SIGGAN_SSIM_MAX_SIZE)
        return FAIL(SIGGAN_E_INVALID, "height = %d outside [%d, %d]", h, SIGGAN_SSIM_MIN_HEIGHT, SIGGAN_SSIM_MAX_SIZE);
    if (w < SIGGAN_SSIM_MIN_WIDTH || w > SIGGAN_SSIM_MAX_SIZE || (w & 3))
        return FAIL(SIGGAN_E_INVALID, "width = %d must be a multiple of 4 in [%d, %d]", w, SIGGAN_SSIM_MIN_WIDTH, SIGGAN_SSIM_MAX_SIZE);
    return SIGGAN_OK;
}

}  // namespace

extern "C" int siggan_ssim_window(float w[SIGGAN_SSIM_TAPS]) {
    if (!w) return FAIL(SIGGAN_E_INVALID, "null window");
    const Taps t = host_taps();
    for (int k = 0; k < TAPS; ++k) w[k] = t.g[k];
    return SIGGAN_OK;
}

extern "C" int64_t siggan_ssim_maps_bytes(int32_t n, int32_t h, int32_t w) {
    if (n < 1) return FAIL(SIGGAN_E_INVALID, "n = %d < 1", n);
    if (int rc = check_size(h, w)) return rc;
    return (int64_t)n * 2 * (h - HALO) * (w - HALO) * (int64_t)sizeof(float);
}

extern "C" int siggan_ssim_prepare_u8(int32_t device, const uint8_t* u8_dev, int32_t n, int32_t h, int32_t w, float* maps_dev,
                                      void* stream) {
    if (n < 1) return FAIL(SIGGAN_E_INVALID, "n = %d < 1", n);
    if (int rc = check_size(h, w)) return rc;
    if (!u8_dev || !maps_dev) return FAIL(SIGGAN_E_INVALID, "null image or map tensor");
    if (int rc = ink_refuse_unaligned({u8_dev, maps_dev}, "u8_dev and maps_dev")) return rc;
    DevGuard dg(device); HIPCHK(dg.err);
    void (*kernel)(Taps, const uint8_t*, int, int, int, float*) = w <= 64 ? k_ssim_prepare<1> : k_ssim_prepare<2>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, host_taps(), u8_dev, n, h, w, maps_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

extern "C" int siggan_ssim_pairs(int32_t device, const uint8_t* a_u8, const float* a_maps, int32_t na, const uint8_t* b_u8,
                                 const float* b_maps, int32_t nb, int32_t h, int32_t w, int32_t mode, float* matrix, float* best,
                                 int32_t* best_index, void* stream) {
    const bool want_best = best || best_index;
    if (int rc = pairs_refuse_counts(na, nb)) return rc;
    if (int rc = check_size(h, w)) return rc;
    if (int rc = pairs_refuse_mode_or_no_output("SIGGAN_SSIM", mode, matrix || want_best)) return rc;
    if (!a_u8 || !a_maps) return FAIL(SIGGAN_E_INVALID, "null a_u8 or a_maps");
    if (int rc = pairs_refuse_same_set("SIGGAN_SSIM", mode, (!b_u8 || b_u8 == a_u8) && (!b_maps || b_maps == a_maps), na, nb, "a's pointers")) return rc;
    if (mode == SIGGAN_SSIM_SAME_SET) { b_u8 = a_u8; b_maps = a_maps; }
    if (!b_u8 || !b_maps) return FAIL(SIGGAN_E_INVALID, "null b_u8 or b_maps");
    if (int rc = pairs_refuse_paired("SIGGAN_SSIM", mode, na, nb, want_best)) return rc;
    if (int rc = ink_refuse_unaligned({a_u8, a_maps, b_u8, b_maps, matrix, best, best_index}, "every pointer")) return rc;

    const int hw = h * w;
    const int RW = hw <= 8192 ? 4 : 2;                                   // a-images (waves) per workgroup: LDS stays under 64 KiB
    int chunk = STAGE_BYTES / hw;
    chunk = chunk < 1 ? 1 : (chunk > MAX_CHUNK ? MAX_CHUNK : chunk);
    const int row_tiles = (na + RW - 1) / RW;
    PairPlan plan{1, nb};
    if (mode == SIGGAN_SSIM_PAIRED) chunk = chunk < RW ? chunk : RW;
    else plan = pair_plan(nb, row_tiles, chunk);                          // whole chunks per split
    const size_t lds = (size_t)RW * 2 * w * sizeof(float) + (size_t)(RW + chunk) * hw;

    DevGuard dg(device); HIPCHK(dg.err);
    hipStream_t st = (hipStream_t)stream;
    void (*kernel)(Taps, const uint8_t*, const float*, int, const uint8_t*, const float*, int, int, int, int, int, int, float*,
                   unsigned long long*) = w <= 64 ? k_ssim_pairs<1> : k_ssim_pairs<2>;
    return pairs_launch<HighestF32>(st, na, plan.S, best, best_index, [&](unsigned long long* keys) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)row_tiles, (unsigned)plan.S), dim3(64 * RW), lds, st, host_taps(), a_u8, a_maps, na, b_u8,
                           b_maps, nb, h, w, mode, chunk, plan.per, matrix, keys);
    });
}
