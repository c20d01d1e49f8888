// dtw.hip -- banded dynamic time warping between column profiles of byte images (include/siggan_dtw.h).  gfx950 only.
//
// k_dtw_profiles: one thread per (image, column) walks the column's rows; neighbouring threads read neighbouring bytes.
// k_dtw_pairs:    a wave64 is a systolic array over the rows of the DP table.  Lane i keeps a's column r0 + i; at step t it
//   owns cell (r0 + i, t - i).  b's columns enter at lane 0 (a readlane of the register image of b, lane index = column) and
//   move one lane per step; `cur` is the lane's own last value D(i, j - 1), `up` arrives from the lane below by the same
//   shift and is D(i - 1, j), and last step's `up` is D(i - 1, j - 1).  A cell outside the band or the grid becomes INF;
//   a cell that exists has an existing predecessor (its diagonal one, or along the first row / column), so INF is never
//   the minimum of an existing cell and never carried into one: the result does not depend on its value.  D(-1, -1) = 0 is
//   lane 0's first diagonal, which makes D(0, 0) = d(0, 0).  Beyond 64 columns the rows go in two strips: lane 63 of the
//   first strip drops D(63, j) into lane j & 63 of one of two `edge` registers (a readlane, then a select on the lane
//   number), and lane 0 of the second strip reads them back as its `up`.  No LDS, no barrier, every lane active throughout.
//   A workgroup of four waves holds four rows of a; a wave walks its slice of b's rows.  The splits of b's rows and a row's
//   `best` as a key (LowestI32) are image_pairs.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_dtw.h"
#include "image_pairs.h"
#include "ink_rows.h"

namespace {

constexpr int INF = 0x3fffffff;          // + a cost (<= 1020) stays far below INT32_MAX
constexpr int WAVES = 4;                 // rows of a per workgroup

__global__ __launch_bounds__(256) void k_dtw_profiles(const uint8_t* __restrict__ u8, int n, int h, int w, int thr,
                                                      uint32_t* __restrict__ prof) {
    const size_t col = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= (size_t)n * w) return;
    const size_t img = col / w;
    const int x = (int)(col - img * w);
    const uint8_t* p = u8 + img * h * w + x;
    int count = 0, top = -1, bottom = -1, runs = 0, before = 0;
    for (int y = 0; y < h; ++y) {
        const int ink = (int)p[(size_t)y * w] < thr;
        count += ink;
        runs += ink & ~before;
        if (ink) {
            top = top < 0 ? y : top;
            bottom = y;
        }
        before = ink;
    }
    if (top < 0) top = bottom = h / 2;
    prof[col] = (uint32_t)count | (uint32_t)top << 8 | (uint32_t)bottom << 16 | (uint32_t)runs << 24;
}

// Every lane takes `src` of the lane below it; lane 0 keeps `first`.  All 64 lanes must be active.
__device__ __forceinline__ int from_below(int first, int src) { return __builtin_amdgcn_update_dpp(first, src, 0x138, 0xf, 0xf, false); }

// Lane `k` (wave-uniform, any value: taken mod 64) of a two-register image of up to 128 entries, entry e in lane e & 63 of register e >> 6.
// The select is between the two VALUES: a select between their addresses sends the pair to LDS (profiles/dtw_resources.md).
template <int NS>
__device__ __forceinline__ int entry(const int (&reg)[NS], int k) {
    const int low = reg[0], high = reg[NS - 1];
    return __builtin_amdgcn_readlane(NS > 1 && (k & 64) ? high : low, k & 63);
}

// DTW of the wave's a (pa: column 64 q + lane in register q, 0 beyond w) with b (pb likewise).  Wave-uniform result.
template <int NS>
__device__ __forceinline__ int dtw_pair(const int (&pa)[NS], const int (&pb)[NS], int w, int band, int lane) {
    int edge[NS];                                                        // D(64 s - 1, .) for the strip s that follows
#pragma unroll
    for (int q = 0; q < NS; ++q) edge[q] = INF;
    int result = 0;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int r0 = 64 * s;
        const int rows = min(64, w - r0);
        const int i = r0 + lane;
        // the columns this strip's rows reach, and per lane the columns its row reaches (none beyond the last row)
        const int jmin = max(0, r0 - band), jmax = min(w - 1, r0 + rows - 1 + band);
        const int lo = max(0, i - band);
        const unsigned reach = i < w ? (unsigned)(min(w - 1, i + band) - lo) : 0u;
        const int lo_or_never = i < w ? lo : w + 64;
        int cur = INF, bcol = 0;
        // lane 0's first diagonal: D(-1, -1) = 0 in the first strip, D(r0 - 1, jmin - 1) after it
        int up = s == 0 ? (lane == 0 ? 0 : INF) : (jmin > 0 ? entry<NS>(edge, jmin - 1) : INF);
        int next[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) next[q] = INF;
        const int last = jmax + rows - 1;
        for (int t = jmin; t <= last; ++t) {
            bcol = from_below(entry<NS>(pb, t), bcol);                   // columns at and beyond w are never used
            const int diag = up;
            up = from_below(s == 0 || t >= w ? INF : entry<NS>(edge, t), cur);
            const int j = t - lane;
            const int d = (int)__builtin_amdgcn_sad_u8((unsigned)pa[s], (unsigned)bcol, 0u);
            const int m = min(min(cur, up), diag);
            cur = (unsigned)(j - lo_or_never) <= reach ? d + m : INF;
            if (s + 1 < NS) {                                            // lane 63 has just finished D(r0 + 63, t - 63)
                const int je = t - 63;
                if (je >= 0) {
                    const int v = __builtin_amdgcn_readlane(cur, 63);
                    const bool mine = lane == (je & 63), high = (je & 64) != 0;
                    next[0] = mine && !high ? v : next[0];
                    next[NS - 1] = mine && high ? v : next[NS - 1];
                }
            }
        }
        if (s + 1 < NS) {
#pragma unroll
            for (int q = 0; q < NS; ++q) edge[q] = next[q];
        } else {
            result = __builtin_amdgcn_readlane(cur, (rows - 1) & 63);    // cell (w - 1, w - 1), finished at the last step
        }
    }
    return result;
}

// grid (ceil(na / WAVES), splits), WAVES waves = a-rows per workgroup.  In PAIRED mode a wave's only column is its own row.
template <int NS>
__global__ __launch_bounds__(64 * WAVES) void k_dtw_pairs(const uint32_t* __restrict__ a_prof, int na, const uint32_t* __restrict__ b_prof,
                                                          int nb, int w, int band, int mode, int per, int32_t* __restrict__ matrix,
                                                          unsigned long long* __restrict__ keys) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int split = blockIdx.y, S = gridDim.y, i = blockIdx.x * WAVES + wave;
    if (i >= na) return;                                                 // wave-uniform; nothing below synchronises waves
    const bool paired = mode == SIGGAN_DTW_PAIRED, same = mode == SIGGAN_DTW_SAME_SET;
    const int j_begin = paired ? i : split * per;
    const int j_end = paired ? i + 1 : min(nb, j_begin + per);
    int pa[NS], pb[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pa[q] = 64 * q + lane < w ? (int)a_prof[(size_t)i * w + 64 * q + lane] : 0;
    unsigned long long best = LowestI32::NONE;
    for (int j = j_begin; j < j_end; ++j) {
        if (same && j == i && !matrix) continue;
#pragma unroll
        for (int q = 0; q < NS; ++q) pb[q] = 64 * q + lane < w ? (int)b_prof[(size_t)j * w + 64 * q + lane] : 0;
        const int value = dtw_pair<NS>(pa, pb, w, band, lane);
        if (matrix && lane == 0) matrix[matrix_slot(paired, i, j, nb)] = value;
        if (!(same && j == i)) keep_better<LowestI32>(best, value, j);
    }
    if (keys && lane == 0) keys[(size_t)i * S + split] = best;
}

int check_width(int32_t w) {
    if (w < 4 || w > SIGGAN_DTW_MAX_SIZE || (w & 3))
        return FAIL(SIGGAN_E_INVALID, "width = %d must be a multiple of 4 in [4, %d]", w, SIGGAN_DTW_MAX_SIZE);
    return SIGGAN_OK;
}

}  // namespace

extern "C" int siggan_dtw_profiles_u8(int32_t device, const uint8_t* u8_dev, int32_t n, int32_t h, int32_t w, int32_t threshold,
                                      uint32_t* profiles_dev, void* stream) {
    if (int rc = ink_refuse_images(u8_dev, profiles_dev ? nullptr : "null profile tensor", n, h, w, SIGGAN_DTW_MAX_SIZE, threshold)) return rc;
    if (int rc = ink_refuse_unaligned({u8_dev, profiles_dev}, "u8_dev and profiles_dev")) return rc;
    DevGuard dg(device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_dtw_profiles, dim3(blocks((int64_t)n * w)), dim3(256), 0, (hipStream_t)stream, u8_dev, n, h, w, threshold,
                       profiles_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}

extern "C" int siggan_dtw_pairs(int32_t device, const uint32_t* a_prof, int32_t na, const uint32_t* b_prof, int32_t nb, int32_t w,
                                int32_t band, int32_t mode, int32_t* matrix, int32_t* best, int32_t* best_index, void* stream) {
    const bool want_best = best || best_index;
    if (int rc = pairs_refuse_counts(na, nb)) return rc;
    if (int rc = check_width(w)) return rc;
    if (band < 0 || band > w - 1) return FAIL(SIGGAN_E_INVALID, "band = %d outside [0, %d]", band, w - 1);
    if (int rc = pairs_refuse_mode_or_no_output("SIGGAN_DTW", mode, matrix || want_best)) return rc;
    if (!a_prof) return FAIL(SIGGAN_E_INVALID, "null a_prof");
    if (int rc = pairs_refuse_same_set("SIGGAN_DTW", mode, !b_prof || b_prof == a_prof, na, nb, "a's pointer")) return rc;
    if (mode == SIGGAN_DTW_SAME_SET) b_prof = a_prof;
    if (!b_prof) return FAIL(SIGGAN_E_INVALID, "null b_prof");
    if (int rc = pairs_refuse_paired("SIGGAN_DTW", mode, na, nb, want_best)) return rc;
    if (int rc = ink_refuse_unaligned({a_prof, b_prof, matrix, best, best_index}, "every pointer")) return rc;

    const int row_tiles = (na + WAVES - 1) / WAVES;
    const PairPlan plan = mode == SIGGAN_DTW_PAIRED ? PairPlan{1, nb} : pair_plan(nb, row_tiles, 1);

    DevGuard dg(device); HIPCHK(dg.err);
    hipStream_t st = (hipStream_t)stream;
    void (*kernel)(const uint32_t*, int, const uint32_t*, int, int, int, int, int, int32_t*, unsigned long long*) =
        w <= 64 ? k_dtw_pairs<1> : k_dtw_pairs<2>;
    return pairs_launch<LowestI32>(st, na, plan.S, best, best_index, [&](unsigned long long* keys) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)row_tiles, (unsigned)plan.S), dim3(64 * WAVES), 0, st, a_prof, na, b_prof, nb, w, band, mode,
                           plan.per, matrix, keys);
    });
}
