// shape.hip -- shape attributes of signature images on the device (include/siggan_shape.h): the ink moments, a quadratic
// objective on them and its gradient with respect to the pixels, in fp64; and the same moments of byte images as exact
// integer sums.  gfx950 only.
//
// One launch, one workgroup of 256 lanes per image.  k_shape_f32<S>: the image is read once (b128 loads) into S * S / 256
// registers per lane -- lane l holds the pixels 4 (256 j + l) + e --, pass 1 forms S0, sum a u, sum a v, pass 2 the central
// second sums with cx, cy known, and a third walk over the registers evaluates the gradient's polynomial in (du, dv) and
// writes dx (b128 stores).  Since 1024 is a multiple of S, a lane's four columns are the same for every j and its row moves
// down by 1024 / S per j.  Every sum: per-lane partial in ascending pixel order, the xor butterfly 32 .. 1 over the wave, the
// four wave sums through LDS in wave order -- every lane ends with the same bits.  k_shape_u8<S>: the same shape in integers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_shape.h"
#include "host.h"

namespace {

constexpr int LANES = 256, WAVES = 4, NF = SIGGAN_SHAPE_FEATURES;

// three fp64 sums at once: butterfly over the wave, then ((w0 + w1) + w2) + w3 through LDS; `sh` is free again on return
__device__ __forceinline__ void fold3(double& a, double& b, double& c, double (*sh)[3], int lane, int wave) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        a = a + __shfl_xor(a, o);
        b = b + __shfl_xor(b, o);
        c = c + __shfl_xor(c, o);
    }
    if (lane == 0) { sh[wave][0] = a; sh[wave][1] = b; sh[wave][2] = c; }
    __syncthreads();
    a = sh[0][0]; b = sh[0][1]; c = sh[0][2];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) { a = a + sh[w][0]; b = b + sh[w][1]; c = c + sh[w][2]; }
    __syncthreads();
}

template <int S>
__global__ __launch_bounds__(LANES) void k_shape_f32(const float* __restrict__ x, const double* __restrict__ weights,
                                                     const double* __restrict__ targets, double* __restrict__ features,
                                                     float* dx, float* __restrict__ objective) {
    constexpr int VEC = S * S / (4 * LANES);          // float4 per lane: 4 or 16
    constexpr int ROW_STEP = 4 * LANES / S;           // rows between a lane's consecutive float4
    constexpr double INV_2S = 1.0 / (2 * S), INV_SS = 1.0 / ((double)S * S);
    __shared__ double sh[WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t img = (size_t)blockIdx.x * (S * S);
    const float4* src = reinterpret_cast<const float4*>(x + img);

    float4 px[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) px[j] = src[j * LANES + tid];

    // the lane's coordinates: columns c0 .. c0 + 3, rows r0 + j * ROW_STEP; u and v are exact in fp64
    const int c0 = (4 * tid) & (S - 1), r0 = (4 * tid) / S;
    double u[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = (double)(2 * (c0 + e) + 1 - S) * INV_2S;

    // ---- pass 1: S0, sum a u, sum a v
    double s0 = 0.0, su = 0.0, sv = 0.0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const double v = (double)(2 * (r0 + j * ROW_STEP) + 1 - S) * INV_2S;
        const float xe[4] = {px[j].x, px[j].y, px[j].z, px[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double a = (1.0 - (double)xe[e]) * 0.5;
            s0 = s0 + a;
            su = su + a * u[e];
            sv = sv + a * v;
        }
    }
    fold3(s0, su, sv, sh, lane, wave);
    const bool empty = !(s0 > 0.0);
    double f[NF];
    f[SIGGAN_SHAPE_MASS] = s0 * INV_SS;
#pragma unroll
    for (int k = 1; k < NF; ++k) f[k] = 0.0;
    double cx = 0.0, cy = 0.0;
    if (!empty) { cx = su / s0; cy = sv / s0; }

    // ---- pass 2: the central second sums
    double du[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) du[e] = u[e] - cx;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const double dv = (double)(2 * (r0 + j * ROW_STEP) + 1 - S) * INV_2S - cy;
        const float xe[4] = {px[j].x, px[j].y, px[j].z, px[j].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double a = (1.0 - (double)xe[e]) * 0.5;
            sxx = sxx + a * (du[e] * du[e]);
            syy = syy + a * (dv * dv);
            sxy = sxy + a * (du[e] * dv);
        }
    }
    fold3(sxx, syy, sxy, sh, lane, wave);
    bool has_slant = false;
    if (!empty) {
        f[SIGGAN_SHAPE_CX] = cx;
        f[SIGGAN_SHAPE_CY] = cy;
        f[SIGGAN_SHAPE_SXX] = sxx / s0;
        f[SIGGAN_SHAPE_SYY] = syy / s0;
        f[SIGGAN_SHAPE_SXY] = sxy / s0;
        has_slant = f[SIGGAN_SHAPE_SYY] > SIGGAN_SHAPE_SYY_MIN;
        if (has_slant) f[SIGGAN_SHAPE_SLANT] = f[SIGGAN_SHAPE_SXY] / f[SIGGAN_SHAPE_SYY];
        f[SIGGAN_SHAPE_SPREAD] = f[SIGGAN_SHAPE_SXX] + f[SIGGAN_SHAPE_SYY];
    }
    if (features && tid == 0) {
#pragma unroll
        for (int k = 0; k < NF; ++k) features[(size_t)blockIdx.x * NF + k] = f[k];
    }
    if (!dx && !objective) return;                    // (the host passes weights and targets with either of them)

    // ---- the objective, and the weighted residuals e_k = w_k (f_k - t_k) of the terms that contribute
    double ek[NF], obj = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const double w = weights[(size_t)blockIdx.x * NF + k];
        const bool on = w != 0.0 && (k == SIGGAN_SHAPE_MASS || !empty) && (k != SIGGAN_SHAPE_SLANT || has_slant);
        double r = 0.0;
        if (on) r = f[k] - targets[(size_t)blockIdx.x * NF + k];   // (a skipped feature's target never enters the arithmetic)
        ek[k] = on ? w * r : 0.0;
        obj = obj + (on ? 0.5 * (w * (r * r)) : 0.0);
    }
    if (objective && tid == 0) objective[blockIdx.x] = (float)obj;
    if (!dx) return;

    // g_p = sum_k e_k df_k/da_p = k0 + ku du + kv dv + kuu du^2 + kvv dv^2 + kuv du dv;  dx_p = -g_p / 2
    double k0 = ek[SIGGAN_SHAPE_MASS] * INV_SS, ku = 0.0, kv = 0.0, kuu = 0.0, kvv = 0.0, kuv = 0.0;
    if (!empty) {
        const double inv = 1.0 / s0;
        const double es = has_slant ? ek[SIGGAN_SHAPE_SLANT] / f[SIGGAN_SHAPE_SYY] : 0.0;      // slant's weight on dsxy
        const double exx = ek[SIGGAN_SHAPE_SXX] + ek[SIGGAN_SHAPE_SPREAD];                      // what multiplies dsxx
        const double eyy = ek[SIGGAN_SHAPE_SYY] + ek[SIGGAN_SHAPE_SPREAD] - es * f[SIGGAN_SHAPE_SLANT];   // ... dsyy
        const double exy = ek[SIGGAN_SHAPE_SXY] + es;                                           // ... dsxy
        ku = ek[SIGGAN_SHAPE_CX] * inv;
        kv = ek[SIGGAN_SHAPE_CY] * inv;
        kuu = exx * inv;
        kvv = eyy * inv;
        kuv = exy * inv;
        k0 = k0 - ((exx * f[SIGGAN_SHAPE_SXX] + eyy * f[SIGGAN_SHAPE_SYY]) + exy * f[SIGGAN_SHAPE_SXY]) * inv;
    }
    float4* dst = reinterpret_cast<float4*>(dx + img);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const double dv = (double)(2 * (r0 + j * ROW_STEP) + 1 - S) * INV_2S - cy;
        const double row = k0 + dv * (kv + kvv * dv);                     // the part every column of the row shares
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double g = row + du[e] * ((ku + kuu * du[e]) + kuv * dv);
            o[e] = (float)(-0.5 * g);
        }
        dst[j * LANES + tid] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

template <int S>
__global__ __launch_bounds__(LANES) void k_shape_u8(const uint8_t* __restrict__ u8, int64_t* __restrict__ sums) {
    constexpr int WORDS = S * S / (4 * LANES);        // 4-byte words per lane: 4 or 16
    constexpr int ROW_STEP = 4 * LANES / S;
    constexpr int NS = SIGGAN_SHAPE_SUMS;
    __shared__ int64_t sh[WAVES][NS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(u8 + (size_t)blockIdx.x * (S * S));
    const int c0 = (4 * tid) & (S - 1), r0 = (4 * tid) / S;
    int32_t acc[NS] = {0, 0, 0, 0, 0, 0};             // at most 64 terms of at most 255 * 127^2 each: below 2.7e8
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        const uint32_t word = src[j * LANES + tid];
        const int q = 2 * (r0 + j * ROW_STEP) + 1 - S;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ink = 255 - (int)((word >> (8 * e)) & 255u), p = 2 * (c0 + e) + 1 - S;
            acc[0] += ink;
            acc[1] += ink * p;
            acc[2] += ink * q;
            acc[3] += ink * p * p;
            acc[4] += ink * q * q;
            acc[5] += ink * p * q;
        }
    }
    int64_t t[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        t[k] = acc[k];
#pragma unroll
        for (int o = 32; o; o >>= 1) t[k] += __shfl_xor(t[k], o);
        if (lane == 0) sh[wave][k] = t[k];
    }
    __syncthreads();
    if (tid < NS) sums[(size_t)blockIdx.x * NS + tid] = ((sh[0][tid] + sh[1][tid]) + sh[2][tid]) + sh[3][tid];
}

}  // namespace

extern "C" int siggan_shape_f32(int32_t device, const float* x_dev, int32_t batch, int32_t s, const double* weights_dev,
                                const double* targets_dev, double* features_dev, float* dx_dev, float* objective_dev, void* stream) {
    if (s != 64 && s != 128) return FAIL(SIGGAN_E_INVALID, "s = %d is not 64 or 128", s);
    if (batch < 1) return FAIL(SIGGAN_E_INVALID, "batch = %d < 1", batch);
    if (!x_dev || (reinterpret_cast<uintptr_t>(x_dev) & 15)) return FAIL(SIGGAN_E_INVALID, "x_dev must be a 16-byte aligned pointer");
    if (!features_dev && !dx_dev && !objective_dev) return FAIL(SIGGAN_E_INVALID, "no output was asked for");
    if ((dx_dev || objective_dev) && (!weights_dev || !targets_dev))
        return FAIL(SIGGAN_E_INVALID, "dx_dev and objective_dev need weights_dev and targets_dev");
    if (reinterpret_cast<uintptr_t>(dx_dev) & 15) return FAIL(SIGGAN_E_INVALID, "dx_dev must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(features_dev) | reinterpret_cast<uintptr_t>(weights_dev) | reinterpret_cast<uintptr_t>(targets_dev)) & 7)
        return FAIL(SIGGAN_E_INVALID, "features_dev, weights_dev and targets_dev must be 8-byte aligned");
    DevGuard dg(device); HIPCHK(dg.err);
    hipStream_t st = (hipStream_t)stream;
    if (s == 64)
        hipLaunchKernelGGL(k_shape_f32<64>, dim3((unsigned)batch), dim3(LANES), 0, st, x_dev, weights_dev, targets_dev, features_dev, dx_dev, objective_dev);
    else
        hipLaunchKernelGGL(k_shape_f32<128>, dim3((unsigned)batch), dim3(LANES), 0, st, x_dev, weights_dev, targets_dev, features_dev, dx_dev, objective_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

extern "C" int siggan_shape_u8(int32_t device, const uint8_t* u8_dev, int32_t batch, int32_t s, int64_t* sums_dev, void* stream) {
    if (s != 64 && s != 128) return FAIL(SIGGAN_E_INVALID, "s = %d is not 64 or 128", s);
    if (batch < 1) return FAIL(SIGGAN_E_INVALID, "batch = %d < 1", batch);
    if (!u8_dev || (reinterpret_cast<uintptr_t>(u8_dev) & 3)) return FAIL(SIGGAN_E_INVALID, "u8_dev must be a 4-byte aligned pointer");
    if (!sums_dev || (reinterpret_cast<uintptr_t>(sums_dev) & 7)) return FAIL(SIGGAN_E_INVALID, "sums_dev must be an 8-byte aligned pointer");
    DevGuard dg(device); HIPCHK(dg.err);
    hipStream_t st = (hipStream_t)stream;
    if (s == 64)
        hipLaunchKernelGGL(k_shape_u8<64>, dim3((unsigned)batch), dim3(LANES), 0, st, u8_dev, sums_dev);
    else
        hipLaunchKernelGGL(k_shape_u8<128>, dim3((unsigned)batch), dim3(LANES), 0, st, u8_dev, sums_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
