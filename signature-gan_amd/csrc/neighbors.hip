// neighbors.hip -- exact fp64 k-nearest-neighbour lists and ball counts between two sets of fp32 rows
// (include/siggan_neighbors.h), on v_mfma_f64_16x16x4_f64.  gfx950 only.
//
// One tile kernel, k_neighbors, with two epilogues.  A workgroup of four waves owns 16 query rows; wave w walks the
// reference tiles w, w + 4, ... of 16 rows each.  Operands, accumulator map and the order of summation are rows_f64.h's:
// the MFMA takes the reference rows as A and the query rows as B, so lane l holds query i0 + (l & 15) against the
// references j0 + (l >> 4) + 4 * reg: one query per lane, hence ONE sorted k-list (distance, row number) per lane, touched
// only when a candidate beats its last entry.
//
// d2 = max(0, (|q|^2 + |r|^2) - 2 q.r).  The norms are the diagonals of the MFMA products R R^T (per reference tile) and
// Q Q^T (once per wave) over the SAME chunk and step order as the dot products: a row against a bit-identical row
// therefore sums the same exact products in the same order three times and gives exactly 0.0.  A VALU sum of squares
// would differ from the MFMA's dot product in the last bits.  The price is a second MFMA per step.
//
// Merging: the four lane groups of a wave by two xor exchanges (16, 32), the four waves through LDS, always by the total
// order (distance, row number) -- row numbers are distinct, so the merged list does not depend on who merges.  Counts are
// integer sums.  No atomics; every output element has one writer.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/siggan_neighbors.h"
#include "host.h"
#include "rows_f64.h"

namespace {

constexpr int WAVES = 4;

__device__ __forceinline__ bool before(double d, int j, double ld, int lj) { return (d < ld) | ((d == ld) & (j < lj)); }

// keep the list sorted by (distance, row number); the last entry drops out.  s runs downwards, so l[s - 1] is still the old
// entry when it moves up.
template <int KC>
__device__ __forceinline__ void insert(double (&ld)[KC], int (&lj)[KC], double d, int j) {
#pragma unroll
    for (int s = KC - 1; s >= 0; --s) {
        const int p = s > 0 ? s - 1 : 0;
        const bool up = s > 0 && before(d, j, ld[p], lj[p]);
        const bool here = before(d, j, ld[s], lj[s]);
        if (up) {
            ld[s] = ld[p];
            lj[s] = lj[p];
        } else if (here) {
            ld[s] = d;
            lj[s] = j;
        }
    }
}

// grid: ceil(nq / 16) workgroups of 256 threads.  COUNT: the ball-count epilogue (KC unused, 1); else the k-list one.
template <int KC, bool VEC, bool COUNT>
__global__ __launch_bounds__(64 * WAVES) void k_neighbors(const float* __restrict__ q, int nq, const float* __restrict__ r, int nr,
                                                          int dim, int k, int exclude_diagonal, double* __restrict__ dist2,
                                                          int32_t* __restrict__ index, const double* __restrict__ radius2,
                                                          int32_t* __restrict__ count) {
    __shared__ double s_d[COUNT ? 1 : WAVES * NT * KC];
    __shared__ int s_j[WAVES * NT * KC];                 // COUNT: the waves' partial counts in the first WAVES * NT words

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = lane & 15, g = lane >> 4;
    const int i = blockIdx.x * NT + x;                   // this lane's query row, as B operand and as C column
    const bool q_ok = i < nq;
    const float* qrow = q + (size_t)(q_ok ? i : 0) * (size_t)dim;

    // |q_i|^2: the diagonal of Q Q^T
    double4_t qq = {0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < dim; c0 += CHUNK) {
        const float4 b = load4<VEC>(qrow, q_ok, c0 + 4 * g, dim);
        chunk_mfma(qq, b, b);
    }
    const double qn = diagonal_of(qq, x);

    double ld[KC];
    int lj[KC];
#pragma unroll
    for (int s = 0; s < KC; ++s) { ld[s] = HUGE_VAL; lj[s] = INT_MAX; }
    int cnt = 0;

    const int tiles = (nr + NT - 1) / NT;
    for (int t = wave; t < tiles; t += WAVES) {
        const int j0 = t * NT;
        const bool r_ok = j0 + x < nr;
        const float* rrow = r + (size_t)(r_ok ? j0 + x : 0) * (size_t)dim;
        double4_t dot = {0.0, 0.0, 0.0, 0.0}, nrm = {0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < dim; c0 += CHUNK) {
            const int kb = c0 + 4 * g;
            const float4 a = load4<VEC>(rrow, r_ok, kb, dim);
            const float4 b = load4<VEC>(qrow, q_ok, kb, dim);
            chunk_mfma_with_norm(dot, nrm, a, b);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int row = g + 4 * reg, j = j0 + row;   // the reference this register holds for query i
            // |r_j|^2 = element (row, row) of R R^T: in the lane of this group whose column is row, same register
            const double rn = __shfl(nrm[reg], (g << 4) | row);
            const double d2 = fmax((qn + rn) - 2.0 * dot[reg], 0.0);
            if (COUNT) {
                if (j < nr && d2 <= radius2[j]) ++cnt;
            } else {
                if (j < nr && !(exclude_diagonal && j == i) && before(d2, j, ld[KC - 1], lj[KC - 1])) insert<KC>(ld, lj, d2, j);
            }
        }
    }

    if (COUNT) {
        cnt += __shfl_xor(cnt, 16);
        cnt += __shfl_xor(cnt, 32);
        if (g == 0) s_j[wave * NT + x] = cnt;
        __syncthreads();
        if (wave == 0 && g == 0 && q_ok) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) total += s_j[w * NT + x];
            count[i] = total;
        }
        return;
    }

    // the four lane groups of the wave: after the two exchanges every group holds the wave's list of query x
#pragma unroll
    for (int step = 16; step <= 32; step <<= 1) {
        double od[KC];
        int oj[KC];
#pragma unroll
        for (int s = 0; s < KC; ++s) { od[s] = __shfl_xor(ld[s], step); oj[s] = __shfl_xor(lj[s], step); }
#pragma unroll
        for (int s = 0; s < KC; ++s)
            if (before(od[s], oj[s], ld[KC - 1], lj[KC - 1])) insert<KC>(ld, lj, od[s], oj[s]);
    }
    if (g == 0) {
#pragma unroll
        for (int s = 0; s < KC; ++s) { s_d[(wave * NT + x) * KC + s] = ld[s]; s_j[(wave * NT + x) * KC + s] = lj[s]; }
    }
    __syncthreads();
    if (wave == 0 && g == 0) {
        for (int w = 1; w < WAVES; ++w)
#pragma unroll
            for (int s = 0; s < KC; ++s) {
                const double d = s_d[(w * NT + x) * KC + s];
                const int j = s_j[(w * NT + x) * KC + s];
                if (before(d, j, ld[KC - 1], lj[KC - 1])) insert<KC>(ld, lj, d, j);
            }
        if (q_ok) {
#pragma unroll
            for (int s = 0; s < KC; ++s)
                if (s < k) {
                    if (dist2) dist2[(size_t)i * k + s] = ld[s];
                    if (index) index[(size_t)i * k + s] = lj[s];
                }
        }
    }
}

template <int KC, bool COUNT>
void launch(bool vec, hipStream_t st, const float* q, int nq, const float* r, int nr, int dim, int k, int excl, double* dist2,
            int32_t* index, const double* radius2, int32_t* count) {
    const dim3 grid((unsigned)((nq + NT - 1) / NT)), block(64 * WAVES);
    if (vec)
        hipLaunchKernelGGL((k_neighbors<KC, true, COUNT>), grid, block, 0, st, q, nq, r, nr, dim, k, excl, dist2, index, radius2, count);
    else
        hipLaunchKernelGGL((k_neighbors<KC, false, COUNT>), grid, block, 0, st, q, nq, r, nr, dim, k, excl, dist2, index, radius2, count);
}

int check_sets(const char* who, const float* q, int nq, const float* r, int nr, int dim) {
    if (!q || !r) return FAIL(SIGGAN_E_INVALID, "%s: null tensor", who);
    if (nq < 1 || nr < 1) return FAIL(SIGGAN_E_INVALID, "%s: nq = %d and nr = %d must be >= 1", who, nq, nr);
    if (dim < 1 || dim > SIGGAN_KNN_MAX_DIM) return FAIL(SIGGAN_E_INVALID, "%s: dim %d outside [1, %d]", who, dim, SIGGAN_KNN_MAX_DIM);
    return SIGGAN_OK;
}

}  // namespace

extern "C" int siggan_knn(int32_t device, const float* q_dev, int32_t nq, const float* r_dev, int32_t nr, int32_t dim, int32_t k,
                          int32_t exclude_diagonal, double* dist2_dev, int32_t* index_dev, void* stream) {
    if (int rc = check_sets("siggan_knn", q_dev, nq, r_dev, nr, dim)) return rc;
    if (!dist2_dev && !index_dev) return FAIL(SIGGAN_E_INVALID, "siggan_knn: null output: dist2_dev and index_dev are both NULL");
    if (k < 1 || k > SIGGAN_KNN_MAX_K) return FAIL(SIGGAN_E_INVALID, "siggan_knn: k = %d outside [1, %d]", k, SIGGAN_KNN_MAX_K);
    const int avail = nr - (exclude_diagonal ? 1 : 0);
    if (k > avail) return FAIL(SIGGAN_E_INVALID, "siggan_knn: k = %d exceeds the %d reference rows a query may take", k, avail);
    DevGuard dg(device); HIPCHK(dg.err);
    const bool vec = rows_allow_16_byte_loads(dim, q_dev, r_dev);
    const hipStream_t st = (hipStream_t)stream;
    const int excl = exclude_diagonal ? 1 : 0;
    if (k == 1)      launch<1, false>(vec, st, q_dev, nq, r_dev, nr, dim, k, excl, dist2_dev, index_dev, nullptr, nullptr);
    else if (k <= 4) launch<4, false>(vec, st, q_dev, nq, r_dev, nr, dim, k, excl, dist2_dev, index_dev, nullptr, nullptr);
    else if (k <= 8) launch<8, false>(vec, st, q_dev, nq, r_dev, nr, dim, k, excl, dist2_dev, index_dev, nullptr, nullptr);
    else             launch<16, false>(vec, st, q_dev, nq, r_dev, nr, dim, k, excl, dist2_dev, index_dev, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

extern "C" int siggan_ball_count(int32_t device, const float* q_dev, int32_t nq, const float* r_dev, int32_t nr, int32_t dim,
                                 const double* radius2_dev, int32_t* count_dev, void* stream) {
    if (int rc = check_sets("siggan_ball_count", q_dev, nq, r_dev, nr, dim)) return rc;
    if (!radius2_dev || !count_dev) return FAIL(SIGGAN_E_INVALID, "siggan_ball_count: null tensor");
    DevGuard dg(device); HIPCHK(dg.err);
    launch<1, true>(rows_allow_16_byte_loads(dim, q_dev, r_dev), (hipStream_t)stream, q_dev, nq, r_dev, nr, dim, 0, 0, nullptr,
                    nullptr, radius2_dev, count_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
