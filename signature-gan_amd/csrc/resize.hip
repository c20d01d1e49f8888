// resize.hip -- Pillow's antialiased bilinear resize for single-channel images (include/siggan_resize.h): the byte path
// that equals Image.resize(size, Image.BILINEAR) for mode 'L' bit for bit, the same linear map on fp32 images and its
// transpose.  gfx950 only.
//
// Tables.  Per axis pair (in, out) the host restates Pillow's precompute_coeffs + normalize_coeffs_8bpc in double, in
// Pillow's operation order (the build has -ffp-contract=off): a window (xmin, length) and ksize weights per output index,
// as 22-bit integers for the byte path and rounded to fp32 for the float paths.  The transposed table lists, per INPUT index,
// the contiguous run of output indices whose window holds it, with the same fp32 weights: the adjoint is then the same
// gather as the forward map with source and destination swapped, so ONE kernel, k_resample, serves all three calls.
//
// k_resample.  A workgroup of 64 x 4 threads owns a tile of the destination: a band of rows times up to 128 columns of one
// image.  Horizontal pass first: the source rows the band's vertical windows reach, resampled to the tile's columns, go to
// LDS in the element type (bytes for the byte path: Pillow's uint8 intermediate, rounding included); after one barrier the
// vertical pass reads them column-wise (lane = column, so a wave reads consecutive LDS addresses).  The intermediate never
// touches memory.  Both passes take four rows at a time: a thread's loads are single bytes (or floats) whose addresses depend
// on a window read just before, and one row at a time is a chain of load latencies with nothing in flight beside it.  Column tiles cost nothing (the horizontal window is read from global memory); row bands repeat the
// halo rows' horizontal pass, so the host takes the fewest bands whose intermediate fits LDS_BUDGET -- for 128x128 -> 64x64
// bytes that is the whole image, 8 KiB, five workgroups' worth per CU next to each other.  Where not even one destination
// row's halo fits (a 1024-row column squeezed into one row), the vertical pass forms each intermediate value on the fly
// instead: the same arithmetic in the same order, hence the same bits, at the price of repeating the horizontal pass per
// vertical tap.  A pass whose axis does not change is skipped, as Pillow skips it; with both skipped the call is a copy.
//
// Plain loads and stores, no atomics; every destination element has one writer and one fixed order of summation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <memory>
#include <new>
#include <vector>

#include "../../include/siggan_resize.h"
#include "host.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;               // Pillow's: 22 bits of weight below an 8-bit pixel, 2 bits of headroom
constexpr int TILE_W = 128;                              // destination columns per workgroup
constexpr int TX = 64, TY = 4;                           // lane = column, wave = row
constexpr size_t LDS_BUDGET = 32 * 1024;                 // intermediate per workgroup: 5 workgroups fit a CU's 160 KiB
constexpr int PLAIN_BAND = 16;                           // destination rows per workgroup when nothing is staged

// ---------------------------------------------------------------------------------------------------------------------
// host: Pillow's coefficients
// ---------------------------------------------------------------------------------------------------------------------

inline double triangle(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

int ksize_of(int in, int out) {
    double filterscale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    return (int)ceil(1.0 * filterscale) * 2 + 1;
}

// bounds (out, 2), w (out, ksize) double: precompute_coeffs for the bilinear filter (support 1.0) over the box [0, in)
void precompute(int in, int out, std::vector<int32_t>& bounds, std::vector<double>& w, int& ksize) {
    double scale, filterscale;
    filterscale = scale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 1.0 * filterscale;
    ksize = (int)ceil(support) * 2 + 1;
    bounds.assign((size_t)out * 2, 0);
    w.assign((size_t)out * ksize, 0.0);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double* k = &w[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            const double v = triangle((x + xmin - center + 0.5) * ss);
            k[x] = v;
            ww += v;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

inline int32_t quantise(double w) {                       // normalize_coeffs_8bpc
    return w < 0.0 ? (int32_t)(-0.5 + w * (1 << PRECISION_BITS)) : (int32_t)(0.5 + w * (1 << PRECISION_BITS));
}

bool sizes_ok(int in, int out) { return in >= 1 && in <= SIGGAN_RESIZE_MAX_IN && out >= 1 && out <= SIGGAN_RESIZE_MAX_OUT; }

// One axis pair on the host and on the device.  fwd: per output index; tr: per input index (the transposed map).
struct AxisTable {
    int in = 0, out = 0, ksize = 0, tk = 0;
    std::vector<int32_t> bounds, tbounds;                 // host copies: the band planner reads them
    void* dev = nullptr;                                  // one allocation holding the five arrays below
    const int32_t *d_bounds = nullptr, *d_kk = nullptr, *d_tbounds = nullptr;
    const float *d_kf = nullptr, *d_tkf = nullptr;
};

// (first, count) must both ascend with the row: the kernel takes a band's first and last row for its halo
bool ascending(const std::vector<int32_t>& b) {
    for (size_t i = 1; i < b.size() / 2; ++i)
        if (b[2 * i] < b[2 * i - 2] || b[2 * i] + b[2 * i + 1] < b[2 * i - 2] + b[2 * i - 1]) return false;
    return true;
}

}  // namespace

struct siggan_resize {
    int device;
    std::vector<std::unique_ptr<AxisTable>> tables;
};

namespace {

int get_table(siggan_resize* ctx, int in, int out, const AxisTable** res) {
    for (const auto& t : ctx->tables)
        if (t->in == in && t->out == out) { *res = t.get(); return SIGGAN_OK; }
    std::unique_ptr<AxisTable> t(new (std::nothrow) AxisTable());
    if (!t) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    std::vector<double> w;
    t->in = in; t->out = out;
    precompute(in, out, t->bounds, w, t->ksize);
    const int ks = t->ksize;
    std::vector<int32_t> kk((size_t)out * ks);
    std::vector<float> kf((size_t)out * ks);
    for (size_t i = 0; i < kk.size(); ++i) { kk[i] = quantise(w[i]); kf[i] = (float)w[i]; }

    // the transposed map: input index i lies in the windows of the outputs first .. first + count - 1
    t->tbounds.assign((size_t)in * 2, 0);
    for (int o = 0; o < out; ++o)
        for (int x = 0; x < t->bounds[2 * o + 1]; ++x) {
            const int i = t->bounds[2 * o] + x;
            if (t->tbounds[2 * i + 1] == 0) t->tbounds[2 * i] = o;
            if (t->tbounds[2 * i] + t->tbounds[2 * i + 1] != o)
                return FAIL(SIGGAN_E_STATE, "siggan_resize: the windows holding input %d of (%d -> %d) are not one run", i, in, out);
            ++t->tbounds[2 * i + 1];
        }
    for (int i = 0; i < in; ++i) {
        if (t->tbounds[2 * i + 1] == 0) t->tbounds[2 * i] = i ? t->tbounds[2 * i - 2] + t->tbounds[2 * i - 1] : 0;   // in no window
        if (t->tbounds[2 * i + 1] > t->tk) t->tk = t->tbounds[2 * i + 1];
    }
    if (t->tk < 1) t->tk = 1;
    if (!ascending(t->bounds) || !ascending(t->tbounds))
        return FAIL(SIGGAN_E_STATE, "siggan_resize: the windows of (%d -> %d) do not ascend", in, out);
    std::vector<float> tkf((size_t)in * t->tk, 0.f);
    for (int i = 0; i < in; ++i)
        for (int j = 0; j < t->tbounds[2 * i + 1]; ++j) {
            const int o = t->tbounds[2 * i] + j;
            tkf[(size_t)i * t->tk + j] = kf[(size_t)o * ks + (i - t->bounds[2 * o])];
        }

    // every array is a whole number of 4-byte words, so the offsets below keep each one aligned
    const size_t nb = sizeof(int32_t) * t->bounds.size(), nk = sizeof(int32_t) * kk.size(), nf = sizeof(float) * kf.size();
    const size_t ntb = sizeof(int32_t) * t->tbounds.size(), ntf = sizeof(float) * tkf.size();
    hipError_t e = hipMalloc(&t->dev, nb + nk + nf + ntb + ntf);
    if (e != hipSuccess) return FAIL(SIGGAN_E_NOMEM, "hipMalloc(%zu) -> %s", nb + nk + nf + ntb + ntf, hipGetErrorString(e));
    char* p = (char*)t->dev;
    const void* srcs[5] = {t->bounds.data(), kk.data(), kf.data(), t->tbounds.data(), tkf.data()};
    const size_t lens[5] = {nb, nk, nf, ntb, ntf};
    char* at[5];
    for (int i = 0; i < 5; ++i) {
        at[i] = p;
        e = hipMemcpy(p, srcs[i], lens[i], hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(t->dev);
            return FAIL(SIGGAN_E_HIP, "siggan_resize: uploading the table of (%d -> %d) -> %s", in, out, hipGetErrorString(e));
        }
        p += lens[i];
    }
    t->d_bounds = (const int32_t*)at[0]; t->d_kk = (const int32_t*)at[1]; t->d_kf = (const float*)at[2];
    t->d_tbounds = (const int32_t*)at[3]; t->d_tkf = (const float*)at[4];
    *res = t.get();
    ctx->tables.push_back(std::move(t));
    return SIGGAN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------------------------------------------

template <typename T> struct Px;
template <> struct Px<uint8_t> {
    typedef int32_t W;                                    // weight and accumulator
    static __device__ __forceinline__ W zero() { return 1 << (PRECISION_BITS - 1); }
    static __device__ __forceinline__ uint8_t fin(W a) {  // clip8: arithmetic shift, then clamp
        const int v = a >> PRECISION_BITS;
        return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
    }
};
template <> struct Px<float> {
    typedef float W;
    static __device__ __forceinline__ W zero() { return 0.f; }
    static __device__ __forceinline__ float fin(W a) { return a; }
};

// one axis of the gather: per destination index (first source index, taps), then k weights
template <typename W> struct Pass {
    const int32_t* bounds;
    const W* w;
    int k;
};

// one element of the horizontal pass: destination column c of a source row
template <typename T>
__device__ __forceinline__ T hpix(const T* __restrict__ row, int c, const Pass<typename Px<T>::W>& ph) {
    typedef typename Px<T>::W W;
    const int first = ph.bounds[2 * c], cnt = ph.bounds[2 * c + 1];
    const W* __restrict__ w = ph.w + (size_t)c * ph.k;
    W a = Px<T>::zero();
    for (int j = 0; j < cnt; ++j) a += (W)row[first + j] * w[j];
    return Px<T>::fin(a);
}

// The horizontal pass down one destination column: source rows r, r + TY, ... < rows of `base` (row pitch ws) into
// dst[r * pitch].  The column's window and weights are read once; four rows go together, so a tap's four loads are in
// flight at once (one row at a time is a chain of dependent load latencies and nothing else).  Per element the sum is
// hpix's: the same taps in the same order.
template <typename T>
__device__ __forceinline__ void hcolumn(const T* __restrict__ base, int ws, int r, int rows, int c, const Pass<typename Px<T>::W>& ph,
                                        T* __restrict__ dst, size_t pitch) {
    typedef typename Px<T>::W W;
    const int first = ph.bounds[2 * c], cnt = ph.bounds[2 * c + 1];
    const W* __restrict__ w = ph.w + (size_t)c * ph.k;
    const size_t step = (size_t)TY * ws;
    for (; r + 3 * TY < rows; r += 4 * TY) {
        const T* __restrict__ p = base + (size_t)r * ws + first;
        W a0 = Px<T>::zero(), a1 = a0, a2 = a0, a3 = a0;
        for (int j = 0; j < cnt; ++j) {
            const W wj = w[j];
            a0 += (W)p[j] * wj;
            a1 += (W)p[step + j] * wj;
            a2 += (W)p[2 * step + j] * wj;
            a3 += (W)p[3 * step + j] * wj;
        }
        dst[(size_t)r * pitch] = Px<T>::fin(a0);
        dst[(size_t)(r + TY) * pitch] = Px<T>::fin(a1);
        dst[(size_t)(r + 2 * TY) * pitch] = Px<T>::fin(a2);
        dst[(size_t)(r + 3 * TY) * pitch] = Px<T>::fin(a3);
    }
    for (; r < rows; r += TY) dst[(size_t)r * pitch] = hpix<T>(base + (size_t)r * ws, c, ph);
}

// grid (n, bands, column tiles), block (64, 4).  has_h / has_v: which passes run (at least one); use_lds: both run and the
// band's intermediate, (halo rows) x (tile columns) elements of T, is staged in dynamic LDS.
template <typename T>
__global__ __launch_bounds__(TX * TY) void k_resample(const T* __restrict__ src, int hs, int ws, T* __restrict__ dst, int hd, int wd,
                                                      Pass<typename Px<T>::W> ph, Pass<typename Px<T>::W> pv, int has_h, int has_v,
                                                      int use_lds, int band) {
    typedef typename Px<T>::W W;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    T* tmp = reinterpret_cast<T*>(s_raw);

    const int tx = threadIdx.x, ty = threadIdx.y;
    const int r0 = blockIdx.y * band, r1 = min(r0 + band, hd);
    const int c0 = blockIdx.z * TILE_W, tw = min(TILE_W, wd - c0);
    const T* __restrict__ img = src + (size_t)blockIdx.x * (size_t)hs * (size_t)ws;
    T* __restrict__ out = dst + (size_t)blockIdx.x * (size_t)hd * (size_t)wd;

    if (!has_v) {                                         // rows pass through: hs == hd
        for (int c = tx; c < tw; c += TX)
            hcolumn<T>(img + (size_t)r0 * ws, ws, ty, r1 - r0, c0 + c, ph, out + (size_t)r0 * wd + c0 + c, (size_t)wd);
        return;
    }

    const int s0 = pv.bounds[2 * r0];                     // the band's halo: source rows s0 .. s0 + rows - 1
    if (use_lds) {
        const int rows = pv.bounds[2 * (r1 - 1)] + pv.bounds[2 * (r1 - 1) + 1] - s0;
        for (int c = tx; c < tw; c += TX) hcolumn<T>(img + (size_t)s0 * ws, ws, ty, rows, c0 + c, ph, tmp + c, (size_t)tw);
        __syncthreads();
        // the vertical pass, four destination rows together for the same reason; a row is one wave's (ty), so the windows
        // and weights are wave-uniform.  j past a row's own window is skipped, not multiplied by a zero weight: the rows
        // it would read may lie outside the halo
        for (int r = r0 + ty; r < r1; r += 4 * TY) {
            int first[4], cnt[4], most = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rq = r + q * TY, ok = rq < r1;
                first[q] = ok ? pv.bounds[2 * rq] - s0 : 0;
                cnt[q] = ok ? pv.bounds[2 * rq + 1] : 0;
                most = max(most, cnt[q]);
            }
            for (int c = tx; c < tw; c += TX) {
                W a[4] = {Px<T>::zero(), Px<T>::zero(), Px<T>::zero(), Px<T>::zero()};
                for (int j = 0; j < most; ++j) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (j < cnt[q]) a[q] += (W)tmp[(first[q] + j) * tw + c] * pv.w[(size_t)(r + q * TY) * pv.k + j];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (r + q * TY < r1) out[(size_t)(r + q * TY) * wd + c0 + c] = Px<T>::fin(a[q]);
            }
        }
        return;
    }
    for (int r = r0 + ty; r < r1; r += TY) {
        const int first = pv.bounds[2 * r], cnt = pv.bounds[2 * r + 1];
        const W* __restrict__ w = pv.w + (size_t)r * pv.k;
        for (int c = tx; c < tw; c += TX) {
            W a = Px<T>::zero();
            if (has_h) {                                  // nothing staged: every intermediate value is formed where it is used
                for (int j = 0; j < cnt; ++j) a += (W)hpix<T>(img + (size_t)(first + j) * ws, c0 + c, ph) * w[j];
            } else {                                      // columns pass through: ws == wd
                for (int j = 0; j < cnt; ++j) a += (W)img[(size_t)(first + j) * ws + c0 + c] * w[j];
            }
            out[(size_t)r * wd + c0 + c] = Px<T>::fin(a);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host: planning and launch
// ---------------------------------------------------------------------------------------------------------------------

// the most halo rows any band of `band` destination rows needs; vb: the vertical pass's (first, count) per destination row
int halo_rows(const std::vector<int32_t>& vb, int hd, int band) {
    int worst = 0;
    for (int r0 = 0; r0 < hd; r0 += band) {
        const int r1 = r0 + band < hd ? r0 + band : hd;
        const int rows = vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1] - vb[2 * r0];
        if (rows > worst) worst = rows;
    }
    return worst;
}

// src (n, hs, ws) -> dst (n, hd, wd); hb / vb: host copies of the passes' bounds (null when the pass is skipped)
template <typename T>
int launch(hipStream_t st, const T* src, int n, int hs, int ws, T* dst, int hd, int wd, Pass<typename Px<T>::W> ph,
           Pass<typename Px<T>::W> pv, const std::vector<int32_t>* hb, const std::vector<int32_t>* vb) {
    const int has_h = hb != nullptr, has_v = vb != nullptr;
    if (!has_h && !has_v) {
        HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n * (size_t)hs * (size_t)ws, hipMemcpyDeviceToDevice, st));
        return SIGGAN_OK;
    }
    const int tile_w = wd < TILE_W ? wd : TILE_W;
    int band = hd < PLAIN_BAND ? hd : PLAIN_BAND, use_lds = 0;
    size_t lds = 0;
    if (has_h && has_v && (size_t)halo_rows(*vb, hd, 1) * tile_w * sizeof(T) <= LDS_BUDGET) {
        use_lds = 1;
        for (int nb = 1; nb <= hd; ++nb) {                // the fewest bands that fit: the halo's horizontal pass is repeated per band
            band = (hd + nb - 1) / nb;
            lds = (size_t)halo_rows(*vb, hd, band) * tile_w * sizeof(T);
            if (lds <= LDS_BUDGET) break;
        }
    }
    const dim3 grid((unsigned)n, (unsigned)((hd + band - 1) / band), (unsigned)((wd + TILE_W - 1) / TILE_W)), block(TX, TY);
    hipLaunchKernelGGL((k_resample<T>), grid, block, lds, st, src, hs, ws, dst, hd, wd, ph, pv, has_h, has_v, use_lds, band);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

int check_call(const char* who, const siggan_resize* ctx, const void* a, const void* b, int n, int h_in, int w_in, int h_out, int w_out) {
    if (!ctx || !a || !b) return FAIL(SIGGAN_E_INVALID, "%s: null argument", who);
    if (n < 1) return FAIL(SIGGAN_E_INVALID, "%s: n must be >= 1, got %d", who, n);
    if (h_in < 1 || h_in > SIGGAN_RESIZE_MAX_IN || w_in < 1 || w_in > SIGGAN_RESIZE_MAX_IN)
        return FAIL(SIGGAN_E_INVALID, "%s: input size %d x %d outside [1, %d]", who, h_in, w_in, SIGGAN_RESIZE_MAX_IN);
    if (h_out < 1 || h_out > SIGGAN_RESIZE_MAX_OUT || w_out < 1 || w_out > SIGGAN_RESIZE_MAX_OUT)
        return FAIL(SIGGAN_E_INVALID, "%s: output size %d x %d outside [1, %d]", who, h_out, w_out, SIGGAN_RESIZE_MAX_OUT);
    return SIGGAN_OK;
}

}  // namespace

extern "C" int siggan_resize_create(int32_t device, siggan_resize** out) {
    if (!out) return FAIL(SIGGAN_E_INVALID, "siggan_resize_create: null argument");
    *out = nullptr;
    DevGuard dg(device); HIPCHK(dg.err);
    siggan_resize* c = new (std::nothrow) siggan_resize();
    if (!c) return FAIL(SIGGAN_E_NOMEM, "out of host memory");
    c->device = device;
    *out = c;
    return SIGGAN_OK;
}

extern "C" int siggan_resize_destroy(siggan_resize* ctx) {
    if (!ctx) return SIGGAN_OK;
    DevGuard dg(ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& t : ctx->tables)
        if (t->dev) (void)hipFree(t->dev);
    delete ctx;
    return SIGGAN_OK;
}

extern "C" int32_t siggan_resize_ksize(int32_t in, int32_t out) {
    if (!sizes_ok(in, out))
        return FAIL(SIGGAN_E_INVALID, "siggan_resize_ksize: (%d -> %d) outside in [1, %d], out [1, %d]", in, out, SIGGAN_RESIZE_MAX_IN,
                    SIGGAN_RESIZE_MAX_OUT);
    return ksize_of(in, out);
}

extern "C" int siggan_resize_table(int32_t in, int32_t out, int32_t* bounds_out, int32_t* kk_out, float* kf_out) {
    if (!sizes_ok(in, out))
        return FAIL(SIGGAN_E_INVALID, "siggan_resize_table: (%d -> %d) outside in [1, %d], out [1, %d]", in, out, SIGGAN_RESIZE_MAX_IN,
                    SIGGAN_RESIZE_MAX_OUT);
    std::vector<int32_t> bounds;
    std::vector<double> w;
    int ksize = 0;
    precompute(in, out, bounds, w, ksize);
    for (size_t i = 0; i < bounds.size(); ++i)
        if (bounds_out) bounds_out[i] = bounds[i];
    for (size_t i = 0; i < w.size(); ++i) {
        if (kk_out) kk_out[i] = quantise(w[i]);
        if (kf_out) kf_out[i] = (float)w[i];
    }
    return SIGGAN_OK;
}

extern "C" int siggan_resize_u8(siggan_resize* ctx, const uint8_t* src_dev, int32_t n, int32_t h_in, int32_t w_in, uint8_t* dst_dev,
                                int32_t h_out, int32_t w_out, void* stream) {
    if (int rc = check_call("siggan_resize_u8", ctx, src_dev, dst_dev, n, h_in, w_in, h_out, w_out)) return rc;
    DevGuard dg(ctx->device); HIPCHK(dg.err);
    const AxisTable *th = nullptr, *tv = nullptr;
    if (w_in != w_out) if (int rc = get_table(ctx, w_in, w_out, &th)) return rc;
    if (h_in != h_out) if (int rc = get_table(ctx, h_in, h_out, &tv)) return rc;
    Pass<int32_t> ph = {th ? th->d_bounds : nullptr, th ? th->d_kk : nullptr, th ? th->ksize : 0};
    Pass<int32_t> pv = {tv ? tv->d_bounds : nullptr, tv ? tv->d_kk : nullptr, tv ? tv->ksize : 0};
    return launch<uint8_t>((hipStream_t)stream, src_dev, n, h_in, w_in, dst_dev, h_out, w_out, ph, pv, th ? &th->bounds : nullptr,
                           tv ? &tv->bounds : nullptr);
}

extern "C" int siggan_resize_f32(siggan_resize* ctx, const float* src_dev, int32_t n, int32_t h_in, int32_t w_in, float* dst_dev,
                                 int32_t h_out, int32_t w_out, void* stream) {
    if (int rc = check_call("siggan_resize_f32", ctx, src_dev, dst_dev, n, h_in, w_in, h_out, w_out)) return rc;
    DevGuard dg(ctx->device); HIPCHK(dg.err);
    const AxisTable *th = nullptr, *tv = nullptr;
    if (w_in != w_out) if (int rc = get_table(ctx, w_in, w_out, &th)) return rc;
    if (h_in != h_out) if (int rc = get_table(ctx, h_in, h_out, &tv)) return rc;
    Pass<float> ph = {th ? th->d_bounds : nullptr, th ? th->d_kf : nullptr, th ? th->ksize : 0};
    Pass<float> pv = {tv ? tv->d_bounds : nullptr, tv ? tv->d_kf : nullptr, tv ? tv->ksize : 0};
    return launch<float>((hipStream_t)stream, src_dev, n, h_in, w_in, dst_dev, h_out, w_out, ph, pv, th ? &th->bounds : nullptr,
                         tv ? &tv->bounds : nullptr);
}

extern "C" int siggan_resize_f32_adjoint(siggan_resize* ctx, const float* dy_dev, int32_t n, int32_t h_out, int32_t w_out, float* dx_dev,
                                         int32_t h_in, int32_t w_in, void* stream) {
    if (int rc = check_call("siggan_resize_f32_adjoint", ctx, dy_dev, dx_dev, n, h_in, w_in, h_out, w_out)) return rc;
    DevGuard dg(ctx->device); HIPCHK(dg.err);
    const AxisTable *th = nullptr, *tv = nullptr;
    if (w_in != w_out) if (int rc = get_table(ctx, w_in, w_out, &th)) return rc;
    if (h_in != h_out) if (int rc = get_table(ctx, h_in, h_out, &tv)) return rc;
    // the transposed tables gather: the source is dy (h_out, w_out), the destination dx (h_in, w_in)
    Pass<float> ph = {th ? th->d_tbounds : nullptr, th ? th->d_tkf : nullptr, th ? th->tk : 0};
    Pass<float> pv = {tv ? tv->d_tbounds : nullptr, tv ? tv->d_tkf : nullptr, tv ? tv->tk : 0};
    return launch<float>((hipStream_t)stream, dy_dev, n, h_out, w_out, dx_dev, h_in, w_in, ph, pv, th ? &th->tbounds : nullptr,
                         tv ? &tv->tbounds : nullptr);
}
