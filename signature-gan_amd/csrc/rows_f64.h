// rows_f64.h -- the fp64 row-tile scheme neighbors.hip and twosample.hip share: products X Y^T of fp32 rows, 16 rows against
// 16 rows, on v_mfma_f64_16x16x4_f64.  gfx950 only.  (moments.hip lays its operands out the other way -- feature per lane,
// row per lane group -- and takes the typedef alone.)
//
// The f64 C/D map is col = l & 15, row = (l >> 4) + 4 * reg -- NOT the f32 16x16 map.  The MFMA takes the j / reference
// rows as A and the i / query rows as B, so lane l holds row i0 + (l & 15) against the rows j0 + (l >> 4) + 4 * reg.
//
// Operands: lane l loads features kb .. kb + 3, kb = c0 + 4 (l >> 4), of row (l & 15) per 16-feature chunk c0 (one 16-byte
// load when the rows allow it) and feeds element e to the chunk's MFMA step e.  Which feature sits in which k slot of a step
// does not matter as long as A and B agree, and they do.  Features past dim and rows past the set load as 0.0.
//
// Norms are diagonals of X X^T over the SAME chunk and step order as the dot products, so a row against a bit-identical row
// sums the same exact products in the same order three times: d2 = (|a|^2 + |b|^2) - 2 a.b is exactly 0.0.  That holds
// across files only because both take the order from here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
constexpr int NT = 16;                                   // tile edge
constexpr int CHUNK = 16;                                // features per K chunk: four MFMA steps of four

// features kb .. kb + 3 of one row; VEC: dim % 4 == 0 and 16-byte aligned bases, so kb < dim covers all four
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, bool row_ok, int kb, int dim) {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (!row_ok) return v;
    if (VEC) {
        if (kb < dim) v = *reinterpret_cast<const float4*>(row + kb);
    } else {
        if (kb < dim) v.x = row[kb];
        if (kb + 1 < dim) v.y = row[kb + 1];
        if (kb + 2 < dim) v.z = row[kb + 2];
        if (kb + 3 < dim) v.w = row[kb + 3];
    }
    return v;
}

// one MFMA step: acc += a b^T over four features, a as A (the j rows) and b as B (the i rows), widened here
__device__ __forceinline__ void step_mfma(double4_t& acc, float a, float b) {
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a, (double)b, acc, 0, 0, 0);
}

// acc += a b^T over one chunk: the four steps x, y, z, w
__device__ __forceinline__ void chunk_mfma(double4_t& acc, const float4& a, const float4& b) {
    step_mfma(acc, a.x, b.x);
    step_mfma(acc, a.y, b.y);
    step_mfma(acc, a.z, b.z);
    step_mfma(acc, a.w, b.w);
}

// dot += a b^T and nrm += a a^T over one chunk, the two products' steps in turn: x, x, y, y, ...  Each accumulator sees
// chunk_mfma's order; taking turns lets one product's MFMA issue while the other's is in flight.
__device__ __forceinline__ void chunk_mfma_with_norm(double4_t& dot, double4_t& nrm, const float4& a, const float4& b) {
    step_mfma(dot, a.x, b.x); step_mfma(nrm, a.x, a.x);
    step_mfma(dot, a.y, b.y); step_mfma(nrm, a.y, a.y);
    step_mfma(dot, a.z, b.z); step_mfma(nrm, a.z, a.z);
    step_mfma(dot, a.w, b.w); step_mfma(nrm, a.w, a.w);
}

// the diagonal element (x, x) of a 16 x 16 product sits in lane ((x & 3) << 4 | x), register x >> 2; -> to every lane of
// column slot x
__device__ __forceinline__ double diagonal_of(const double4_t& acc, int x) {
    const int src = ((x & 3) << 4) | x;
    const double d0 = __shfl(acc[0], src), d1 = __shfl(acc[1], src), d2 = __shfl(acc[2], src), d3 = __shfl(acc[3], src);
    const int reg = x >> 2;
    return reg == 0 ? d0 : reg == 1 ? d1 : reg == 2 ? d2 : d3;
}

// load4<true> is allowed: whole float4s per row, and every row of the one or two sets starts on 16 bytes
inline bool rows_allow_16_byte_loads(int dim, const float* p0, const float* p1 = nullptr) {
    return (dim & 3) == 0 && ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1)) & 15) == 0;
}

}  // namespace
