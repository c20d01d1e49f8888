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
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <new>

#include "../../include/siggan_verifier.h"
#include "host.h"
#include "verifier_parts.h"

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
// thread = (pooled pixel, 8 output channels); block = 64 pooled pixels x 4 channel groups.  Images [0, nsplit) come from
// x1, the rest from x2.  out: (N, 32, 32, 32) NHWC.
template <bool U8>
__global__ __launch_bounds__(256) void k_vconv1(const void* __restrict__ x1, const void* __restrict__ x2, int nsplit,
                                                const float* __restrict__ w /* (32, 25) */, const float* __restrict__ sc,
                                                const float* __restrict__ sh, float* __restrict__ out) {
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
    }
}

// ---------------------------------------------------------------- conv2 / conv3: implicit GEMM + affine + ReLU + pool
// x: (N, H, H, CI) NHWC; wp: [CO][KS*KS*CI]; out: (N, H/2, H/2, CO).  conv_tile's 128 x 64 block tile over rows in pooling-window
// order (PoolRows): registers 4g..4g+3 of an accumulator are one window, so the max is taken in registers.
template <int KS, int CI, int CO, int H>
__global__ __launch_bounds__(256) void k_vconv(const float* __restrict__ x, const float* __restrict__ wp,
                                               const float* __restrict__ sc, const float* __restrict__ sh,
                                               float* __restrict__ out) {
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
                                               int nsplit) {
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
}

// ---------------------------------------------------------------- pair head (one 64-thread block per pair)
__global__ __launch_bounds__(64) void k_vhead(const float* __restrict__ e1, const float* __restrict__ e2, int E,
                                              const float* __restrict__ w0 /* (64, E) */, const float* __restrict__ b0,
                                              const float* __restrict__ w3 /* (64) */, const float* __restrict__ b3,
                                              float* __restrict__ score) {
    extern __shared__ float sd[];                      // E differences
    const int p = blockIdx.x, j = threadIdx.x;
    for (int k = j; k < E; k += VHID) sd[k] = fabsf(e1[(size_t)p * E + k] - e2[(size_t)p * E + k]);
    __syncthreads();
    const float* wr = w0 + (size_t)j * E;
    float a = 0.f;
    for (int k = 0; k < E; ++k) a = fmaf(sd[k], wr[k], a);
    a = fmaxf(a + b0[j], 0.f);
    const float logit = wave_sum(a * w3[j]) + b3[0];
    if (j == 0) score[p] = 1.0f / (1.0f + expf(-logit));
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
    v->device = device; v->E = E; v->Nmax = max_images; v->bound = false; v->last_n = 0; v->ws = nullptr;
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
    delete v;
    return SIGGAN_OK;
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
    if (hipGetLastError() != hipSuccess) return FAIL(SIGGAN_E_HIP, "siggan_verifier_bind: kernel launch failed");
    v->bound = true;
    return SIGGAN_OK;
}

// the encoder over n images (the first nsplit from x1, the rest from x2); embeddings to out1 / out2 likewise
static int encode(siggan_verifier* v, const void* x1, const void* x2, int fmt, int n, int nsplit, float* out1, float* out2,
                  hipStream_t s) {
    if (fmt == SIGGAN_VFMT_U8)
        hipLaunchKernelGGL(k_vconv1<true>, dim3(n * 16), dim3(256), 0, s, x1, x2, nsplit, v->w1, v->sc1, v->sh1, v->pool1);
    else
        hipLaunchKernelGGL(k_vconv1<false>, dim3(n * 16), dim3(256), 0, s, x1, x2, nsplit, v->w1, v->sc1, v->sh1, v->pool1);
    hipLaunchKernelGGL((k_vconv<5, 32, 64, 32>), dim3(n * 1024 / 128, 1), dim3(256), 0, s, v->pool1, v->wp2, v->sc2, v->sh2, v->pool2);
    hipLaunchKernelGGL((k_vconv<3, 64, 128, 16>), dim3(n * 256 / 128, 2), dim3(256), 0, s, v->pool2, v->wp3, v->sc3, v->sh3, v->pool3);
    hipLaunchKernelGGL(k_vfc1, dim3(VFC1_N / 64, (n + 63) / 64, VFC1_SPLIT), dim3(256), 0, s, v->pool3, v->wfc1, v->part, n);
    hipLaunchKernelGGL(k_vtail, dim3(n), dim3(256), (size_t)v->E * 4, s, v->part, n, v->bfc1, v->wfc2, v->bfc2, v->E, v->fc1, out1,
                       out2, nsplit);
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
    return encode(v, x, x, fmt, n, n, emb, emb, (hipStream_t)stream);
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
    if ((rc = encode(v, x1, x2, fmt, 2 * np, np, o1, o2, s))) return rc;
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
