// row_d2.h -- the row-difference squared distance diverse.hip and kmeans.hip share (include/siggan_diverse.h states it):
// d2 = sum_k (xi[k] - xp[k])^2 in fp64 over the widened fp32 values, formed as differences, so identical rows give exactly
// 0.0.  Order, fixed: lane l adds the squares of the features k = l, l + 64, ... ascending from 0.0, then the 64 lane sums
// fold by the xor butterfly 32 .. 1.  a + b == b + a, so every lane returns the same bits.  No fused multiply-add (the
// library is built with -ffp-contract=off).  Both files give the same bits only because both take the order from here.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// one whole wave per call; xi: a row in global memory, xp: the other row (the callers stage it in LDS)
__device__ __forceinline__ double wave_row_d2(const float* __restrict__ xi, const float* xp, int dim, int lane) {
    double acc = 0.0;
    for (int k = lane; k < dim; k += 64) {
        const double d = (double)xi[k] - (double)xp[k];
        acc = acc + d * d;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) acc = acc + __shfl_xor(acc, o);
    return acc;
}

}  // namespace
