// diverse.hip -- greedy farthest-point selection on the device (include/siggan_diverse.h): the acting half of the diversity
// metrics.  gfx950 only.
//
// One plain launch per pick, enqueued blindly; no workgroup waits for another.  A workgroup (four waves) owns ROWS
// consecutive rows, wave w the rows [w * ROWS / 4, (w + 1) * ROWS / 4) of them.
// k_diverse_init: m = anchor_d2 or +inf, taken = 0, the first partials (buffer 0), the forced first row's m.
// k_diverse_pick (launch t): prologue -- every workgroup folds the partials of buffer t & 1 into the pick p under the total
//   order "larger m, then lower row" (or takes the forced first), and leaves when the selection has stopped; workgroup 0
//   records order[t] / gain2[t], or the count at a stop.  Body -- row p goes to LDS, every wave forms d2(i, p) for its rows
//   with lanes across features (lane l: k = l, l + 64, ... ascending, then the xor butterfly 32 .. 1), m[i] = min(m[i], d2),
//   and the workgroup's best not-taken eligible row becomes its partial in buffer (t + 1) & 1.
//   A stop is a marker row in the partials, copied forward by every workgroup: there is no word one workgroup writes while
//   another reads it.
// k_diverse_tail: order / gain2 beyond the count, the count, min_d2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/siggan_diverse.h"
#include "host.h"
#include "row_d2.h"

namespace {

constexpr int ROWS = SIGGAN_DIVERSE_ROW_TILE, WAVES = 4, WAVE_ROWS = ROWS / WAVES;
constexpr int NO_ROW = -1, STOPPED = -2;

struct Partial { double val; int32_t row; int32_t pad; };        // a workgroup's best candidate; row NO_ROW: it has none
struct State { double first_gain; int32_t count; int32_t pad; }; // m[first] before any pick; the count at a stop, -1: none yet

struct Layout { size_t m, taken, part, state, bytes; int groups; };
Layout layout(int n) {
    Layout l;
    l.groups = (n + ROWS - 1) / ROWS;
    l.m = 0;
    l.taken = l.m + sizeof(double) * (size_t)n;
    l.part = l.taken + (((size_t)n + 15) & ~(size_t)15);
    l.state = l.part + 2 * sizeof(Partial) * (size_t)l.groups;
    l.bytes = l.state + sizeof(State);
    return l;
}

// the total order of candidates: a larger m first, equal m (+inf included) by the lower row; NO_ROW (m = -1) loses to all
__device__ __forceinline__ bool before(double va, int ra, double vb, int rb) {
    return va > vb || (va == vb && (unsigned)ra < (unsigned)rb);
}
__device__ __forceinline__ void wave_best(double& v, int& r) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double v2 = __shfl_xor(v, o);
        const int r2 = __shfl_xor(r, o);
        if (before(v2, r2, v, r)) { v = v2; r = r2; }
    }
}

__global__ __launch_bounds__(64) void k_diverse_init(int n, const uint8_t* __restrict__ eligible, const double* __restrict__ anchor,
                                                     int first, double* __restrict__ m, uint8_t* __restrict__ taken,
                                                     Partial* __restrict__ part, State* __restrict__ state) {
    const int lane = threadIdx.x, i = blockIdx.x * ROWS + lane;
    double v = -1.0;
    int r = NO_ROW;
    if (lane < ROWS && i < n) {
        const double a = anchor ? anchor[i] : INFINITY;
        m[i] = a;
        taken[i] = 0;
        if (i == first) state->first_gain = a;
        if (!eligible || eligible[i]) { v = a; r = i; }
    }
    wave_best(v, r);
    if (lane == 0) {
        Partial out; out.val = v; out.row = r; out.pad = 0;
        part[blockIdx.x] = out;
        if (blockIdx.x == 0) state->count = -1;
    }
}

__global__ __launch_bounds__(256) void k_diverse_pick(const float* __restrict__ x, int n, int dim, const uint8_t* __restrict__ eligible,
                                                      double* __restrict__ m, uint8_t* __restrict__ taken,
                                                      const Partial* __restrict__ cur, Partial* __restrict__ next, int groups,
                                                      State* __restrict__ state, int t, int first, double min_gain2,
                                                      int32_t* __restrict__ order, double* __restrict__ gain2) {
    __shared__ float xp[SIGGAN_DIVERSE_MAX_DIM];
    __shared__ double wv[WAVES];
    __shared__ int wr[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    Partial out; out.pad = 0;

    // ---- prologue: which row is pick t?  (every exit below is taken by the whole workgroup)
    int p;
    double gain;
    if (cur[0].row == STOPPED) {                                          // stopped in an earlier launch: pass the marker on
        if (tid == 0) { out.val = -1.0; out.row = STOPPED; next[blockIdx.x] = out; }
        return;
    }
    if (t == 0 && first >= 0) {
        p = first;
        gain = state->first_gain;
    } else {
        double v = -1.0;
        int r = NO_ROW;
        for (int g = tid; g < groups; g += 256) {
            const Partial c = cur[g];
            if (before(c.val, c.row, v, r)) { v = c.val; r = c.row; }
        }
        wave_best(v, r);
        if (lane == 0) { wv[wave] = v; wr[wave] = r; }
        __syncthreads();
        v = wv[0]; r = wr[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
            if (before(wv[w], wr[w], v, r)) { v = wv[w]; r = wr[w]; }
        __syncthreads();                                                  // wv / wr are written again below
        p = r;
        gain = v;
        if (p < 0 || gain < min_gain2) {                                  // nothing left, or nothing far enough: stop at t
            if (tid == 0) {
                out.val = -1.0; out.row = STOPPED; next[blockIdx.x] = out;
                if (blockIdx.x == 0) state->count = t;
            }
            return;
        }
    }
    if (blockIdx.x == 0 && tid == 0) { order[t] = p; gain2[t] = gain; }

    // ---- body: m[i] = min(m[i], d2(i, p)) for this workgroup's rows, and its best remaining candidate
    const float* xrow = x + (size_t)p * dim;
    for (int k = tid; k < dim; k += 256) xp[k] = xrow[k];
    __syncthreads();
    double bv = -1.0;
    int br = NO_ROW;
    const int base = blockIdx.x * ROWS + wave * WAVE_ROWS;
    for (int j = 0; j < WAVE_ROWS; ++j) {
        const int i = base + j;                                           // wave-uniform
        if (i >= n) break;
        const float* xi = x + (size_t)i * dim;
        const double acc = wave_row_d2(xi, xp, dim, lane);                // row_d2.h: every lane holds the same bits
        double mi = m[i];
        mi = acc < mi ? acc : mi;
        const bool gone = i == p || taken[i] != 0;
        if (lane == 0) {
            m[i] = mi;
            if (i == p) taken[i] = 1;
        }
        if (!gone && (!eligible || eligible[i]) && before(mi, i, bv, br)) { bv = mi; br = i; }
    }
    if (lane == 0) { wv[wave] = bv; wr[wave] = br; }
    __syncthreads();
    if (tid == 0) {
        double v = wv[0];
        int r = wr[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w)
            if (before(wv[w], wr[w], v, r)) { v = wv[w]; r = wr[w]; }
        out.val = v; out.row = r;
        next[blockIdx.x] = out;
    }
}

__global__ __launch_bounds__(256) void k_diverse_tail(int n, int n_select, const double* __restrict__ m, const State* __restrict__ state,
                                                      int32_t* __restrict__ order, double* __restrict__ gain2,
                                                      int32_t* __restrict__ count, double* __restrict__ min_d2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int c = state->count;
    if (c < 0) c = n_select;
    if (i >= c && i < n_select) { order[i] = -1; gain2[i] = 0.0; }
    if (i == 0) count[0] = c;
    if (min_d2 && i < n) min_d2[i] = m[i];
}

}  // namespace

extern "C" size_t siggan_select_diverse_workspace(int32_t n) {
    if (n < 1 || n > SIGGAN_DIVERSE_MAX_N) return 0;
    return layout(n).bytes;
}

extern "C" int siggan_select_diverse(int32_t device, const float* x_dev, int32_t n, int32_t dim, const uint8_t* eligible_dev,
                                     const double* anchor_d2_dev, int32_t first, int32_t n_select, double min_gain2,
                                     int32_t* order_dev, double* gain2_dev, int32_t* count_dev, double* min_d2_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!x_dev || !order_dev || !gain2_dev || !count_dev || !workspace_dev) return FAIL(SIGGAN_E_INVALID, "null tensor");
    if (n < 1 || n > SIGGAN_DIVERSE_MAX_N) return FAIL(SIGGAN_E_INVALID, "n = %d outside [1, %d]", n, SIGGAN_DIVERSE_MAX_N);
    if (dim < 1 || dim > SIGGAN_DIVERSE_MAX_DIM) return FAIL(SIGGAN_E_INVALID, "dim = %d outside [1, %d]", dim, SIGGAN_DIVERSE_MAX_DIM);
    if (n_select < 1 || n_select > n) return FAIL(SIGGAN_E_INVALID, "n_select = %d outside [1, n = %d]", n_select, n);
    if (first < -1 || first >= n) return FAIL(SIGGAN_E_INVALID, "first = %d outside [-1, n = %d)", first, n);
    if (!(min_gain2 >= 0.0)) return FAIL(SIGGAN_E_INVALID, "min_gain2 must be >= 0, got %g", min_gain2);
    const Layout l = layout(n);
    if (workspace_bytes < l.bytes)
        return FAIL(SIGGAN_E_INVALID, "workspace of %zu bytes, %zu needed (siggan_select_diverse_workspace)", workspace_bytes, l.bytes);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 7) return FAIL(SIGGAN_E_INVALID, "workspace_dev must be 8-byte aligned");
    DevGuard dg(device); HIPCHK(dg.err);
    char* ws = static_cast<char*>(workspace_dev);
    double* m = reinterpret_cast<double*>(ws + l.m);
    uint8_t* taken = reinterpret_cast<uint8_t*>(ws + l.taken);
    Partial* part[2] = {reinterpret_cast<Partial*>(ws + l.part), reinterpret_cast<Partial*>(ws + l.part) + l.groups};
    State* state = reinterpret_cast<State*>(ws + l.state);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_diverse_init, dim3((unsigned)l.groups), dim3(64), 0, s, n, eligible_dev, anchor_d2_dev, first, m, taken, part[0], state);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < n_select; ++t) {
        hipLaunchKernelGGL(k_diverse_pick, dim3((unsigned)l.groups), dim3(256), 0, s, x_dev, n, dim, eligible_dev, m, taken,
                           (const Partial*)part[t & 1], part[(t + 1) & 1], l.groups, state, t, first, min_gain2, order_dev, gain2_dev);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_diverse_tail, dim3(blocks(n)), dim3(256), 0, s, n, n_select, (const double*)m, (const State*)state, order_dev,
                       gain2_dev, count_dev, min_d2_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
