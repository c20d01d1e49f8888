// kmeans.hip -- k-means++ seeding and Lloyd passes on fp32 rows, in fp64 (include/siggan_kmeans.h).  gfx950 only.
//
// Everything is plain launches enqueued blindly; ordering comes from the stream, no workgroup waits for another, and every
// sum has one fixed order (the header's two-level sum: 64-row blocks ascending, then the blocks ascending).
// Seeding, step s >= 1:
//   k_seed_update: a workgroup of four waves per 64-row block; the previous pick (centres[s - 1]) goes to LDS, every wave forms
//     d2(i, pick) for 16 rows with lanes across features (row_d2.h, diverse.hip's order), m[i] = min(m[i], d2), and one
//     thread adds the block's 64 values of m in ascending order into S_b.  At s == 1 the old m counts as +inf.
//   k_seed_pick: one workgroup.  One thread folds the S_b into the Q_b (LDS), target = u_s * T, the first block with
//     Q_b > target is found by all threads, one thread walks that block's prefix, all threads copy the row.
// Lloyd, pass t: siggan_knn (k = 1) writes label and mind2; k_lloyd_stats counts the changed labels and sums mind2 per
//   64-row block; k_lloyd_fold folds both; k_lloyd_update gives a workgroup one (centre, slab of 256 features) pair: it walks
//   the label array in 64-row steps, a ballot says which of the 64 rows belong to the centre, and thread f adds x[i][f]
//   for those rows in ascending i.  The same walk counts the centre's rows, so after the last assignment the kernel runs
//   once more with one wave per centre and no sums.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/siggan_kmeans.h"
#include "../../include/siggan_neighbors.h"
#include "host.h"
#include "rng.h"
#include "row_d2.h"

namespace {

constexpr int SB = SIGGAN_KMEANS_SUM_BLOCK, SLAB = SIGGAN_KMEANS_FEATURE_SLAB;
constexpr int MAX_BLOCKS = SIGGAN_KMEANS_MAX_N / SB, WAVES = 4, WAVE_ROWS = SB / WAVES;
static_assert(SB == 64, "a block of the two-level sum is one wave's worth of rows");
static_assert(SIGGAN_KMEANS_MAX_K <= 256, "k_seed_pick tests one candidate row per thread");

// v: m of the seeding, or mind2 when the caller of the Lloyd passes wants none; sums: S_b; prev: last pass's labels;
// part: changed labels per block
struct Layout { size_t v, sums, prev, part, bytes; int blocks; };
Layout layout(int n) {
    Layout l;
    l.blocks = (n + SB - 1) / SB;
    l.v = 0;
    l.sums = l.v + sizeof(double) * (size_t)n;
    l.prev = l.sums + sizeof(double) * (size_t)l.blocks;
    l.part = l.prev + ((sizeof(int32_t) * (size_t)n + 7) & ~(size_t)7);
    l.bytes = l.part + ((sizeof(int32_t) * (size_t)l.blocks + 7) & ~(size_t)7);
    return l;
}

// ------------------------------------------------------------------------------------------------------------ seeding
// grid: ceil(n / 64) workgroups of 256 threads
__global__ __launch_bounds__(64 * WAVES) void k_seed_update(const float* __restrict__ x, int n, int dim, const float* __restrict__ pick,
                                                            int first, double* __restrict__ m, double* __restrict__ sums) {
    __shared__ float xp[SIGGAN_KMEANS_MAX_DIM];
    __shared__ double mb[SB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int k = tid; k < dim; k += 64 * WAVES) xp[k] = pick[k];
    __syncthreads();
    const int base = blockIdx.x * SB;
    for (int j = 0; j < WAVE_ROWS; ++j) {
        const int r = wave * WAVE_ROWS + j, i = base + r;               // wave-uniform
        if (i >= n) break;
        const double d2 = wave_row_d2(x + (size_t)i * dim, xp, dim, lane);
        if (lane == 0) {
            double mi = first ? INFINITY : m[i];
            mi = d2 < mi ? d2 : mi;
            m[i] = mi;
            mb[r] = mi;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int rows = n - base < SB ? n - base : SB;
        double s = 0.0;
        for (int r = 0; r < rows; ++r) s = s + mb[r];
        sums[blockIdx.x] = s;
    }
}

// grid: one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_seed_pick(const float* __restrict__ x, int n, int dim, int s, unsigned long long seed,
                                                   const double* __restrict__ m, const double* __restrict__ sums, int blocks,
                                                   float* __restrict__ centres, int32_t* __restrict__ seed_rows) {
    __shared__ double q[MAX_BLOCKS];
    __shared__ double s_total, s_target;
    __shared__ int s_row, s_blk;
    const int tid = threadIdx.x;
    const uint4 w = siggan::draw_raw(seed, (unsigned long long)s, 0, SIGGAN_KMEANS_STREAM);
    const double u = ((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) * (1.0 / 9007199254740992.0);   // exact
    if (s == 0) {
        if (tid == 0) s_row = (int)floor(u * (double)n);
    } else {
        for (int b = tid; b < blocks; b += 256) q[b] = sums[b];
        __syncthreads();
        if (tid == 0) {
            double a = 0.0;
            for (int b = 0; b < blocks; ++b) { a = a + q[b]; q[b] = a; }
            s_total = a;
            s_target = u * a;
            s_blk = blocks;
            s_row = a == 0.0 ? INT_MAX : -1;                           // a minimum resp. a maximum is taken below
        }
        __syncthreads();
        const double target = s_target;
        if (s_total == 0.0) {
            // every row coincides with a chosen one: the lowest row number not chosen so far is among 0 .. s (s < k <= n)
            bool chosen = tid > s;
            for (int j = 0; j < s; ++j) chosen |= seed_rows[j] == tid;
            if (!chosen) atomicMin(&s_row, tid);                       // LDS
        } else {
            for (int b = tid; b < blocks; b += 256)
                if (q[b] > target) atomicMin(&s_blk, b);               // LDS
            __syncthreads();
            const int blk = s_blk;
            if (blk < blocks) {
                if (tid == 0) {                                        // Q_blk > target: some prefix inside the block is
                    const double before = blk ? q[blk - 1] : 0.0;
                    const int base = blk * SB, rows = n - base < SB ? n - base : SB;
                    double r = 0.0;
                    int row = base + rows - 1;
                    for (int i = 0; i < rows; ++i) {
                        r = r + m[base + i];
                        if (before + r > target) { row = base + i; break; }
                    }
                    s_row = row;
                }
            } else {                                                   // u * T rounded up to T: the last row with weight
                int best = -1;
                for (int i = tid; i < n; i += 256)
                    if (m[i] > 0.0) best = i;
                atomicMax(&s_row, best);                               // LDS
            }
        }
    }
    __syncthreads();
    int row = s_row;
    row = row < 0 ? 0 : row > n - 1 ? n - 1 : row;                     // step 0's min(n - 1, .); otherwise no change
    const float* src = x + (size_t)row * dim;
    float* dst = centres + (size_t)s * dim;
    for (int k = tid; k < dim; k += 256) dst[k] = src[k];
    if (tid == 0) seed_rows[s] = row;
}

// -------------------------------------------------------------------------------------------------------------- Lloyd
// grid: ceil(n / 64) workgroups of one wave
__global__ __launch_bounds__(64) void k_lloyd_stats(const int32_t* __restrict__ label, const double* __restrict__ mind2,
                                                    int32_t* __restrict__ prev, int n, int first, double* __restrict__ sums,
                                                    int32_t* __restrict__ part) {
    const int lane = threadIdx.x, base = blockIdx.x * SB, i = base + lane;
    const bool ok = i < n;
    const int lab = ok ? label[i] : -1;
    const int old = ok && !first ? prev[i] : -1;
    if (ok) prev[i] = lab;
    const int changed = __popcll(__ballot(ok && lab != old));
    const double v = ok ? mind2[i] : 0.0;
    const int rows = n - base < SB ? n - base : SB;
    double s = 0.0;
    for (int r = 0; r < rows; ++r) s = s + __shfl(v, r);
    if (lane == 0) { sums[blockIdx.x] = s; part[blockIdx.x] = changed; }
}

// grid: one workgroup of 256 threads
__global__ __launch_bounds__(256) void k_lloyd_fold(const double* __restrict__ sums, const int32_t* __restrict__ part, int blocks,
                                                    double* __restrict__ inertia, int32_t* __restrict__ changed) {
    __shared__ double q[MAX_BLOCKS];
    __shared__ int s_changed;
    const int tid = threadIdx.x;
    if (tid == 0) s_changed = 0;
    int c = 0;
    for (int b = tid; b < blocks; b += 256) { q[b] = sums[b]; c += part[b]; }
    __syncthreads();
    atomicAdd(&s_changed, c);                                          // LDS; integers: the order cannot show
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int b = 0; b < blocks; ++b) a = a + q[b];
        inertia[0] = a;
        changed[0] = s_changed;
    }
}

// grid: (k, ceil(dim / 256)) workgroups of 256 threads with do_update; (k, 1) workgroups of 64 threads without
__global__ __launch_bounds__(SLAB) void k_lloyd_update(const float* __restrict__ x, int n, int dim, const int32_t* __restrict__ label,
                                                       float* __restrict__ centres, int32_t* __restrict__ count, int do_update) {
    const int tid = threadIdx.x, lane = tid & 63, j = blockIdx.x;
    const int f = blockIdx.y * SLAB + tid;
    if (f - lane >= dim) return;                                       // a whole wave past the last feature (never wave 0 of slab 0)
    const bool live = f < dim;
    const float* col = x + (live ? f : 0);
    double acc = 0.0;
    int cnt = 0;
    int lab = lane < n ? label[lane] : -1;
    for (int base = 0; base < n; base += 64) {
        const int ahead = base + 64 + lane;
        const int next = ahead < n ? label[ahead] : -1;                // the next step's labels, in flight during this one
        unsigned long long mask = __ballot(lab == j);                  // wave-uniform: the rows of this step that belong to j
        cnt += __popcll(mask);
        while (do_update && mask) {
            // up to four rows' loads go out together; the adds keep the ascending row order
            const int r0 = __ffsll(mask) - 1; mask &= mask - 1;
            const bool h1 = mask != 0;
            const int r1 = h1 ? __ffsll(mask) - 1 : r0; mask &= mask - (h1 ? 1 : 0);
            const bool h2 = mask != 0;
            const int r2 = h2 ? __ffsll(mask) - 1 : r0; mask &= mask - (h2 ? 1 : 0);
            const bool h3 = mask != 0;
            const int r3 = h3 ? __ffsll(mask) - 1 : r0; mask &= mask - (h3 ? 1 : 0);
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            if (live) {
                v0 = col[(size_t)(base + r0) * dim];
                if (h1) v1 = col[(size_t)(base + r1) * dim];
                if (h2) v2 = col[(size_t)(base + r2) * dim];
                if (h3) v3 = col[(size_t)(base + r3) * dim];
            }
            acc = acc + (double)v0;
            if (h1) acc = acc + (double)v1;
            if (h2) acc = acc + (double)v2;
            if (h3) acc = acc + (double)v3;
        }
        lab = next;
    }
    if (do_update && live && cnt > 0) centres[(size_t)j * dim + f] = (float)(acc / (double)cnt);
    if (blockIdx.y == 0 && tid == 0) count[j] = cnt;
}

int check_sizes(const char* who, int n, int dim, int k, const void* workspace, size_t workspace_bytes) {
    if (n < 1 || n > SIGGAN_KMEANS_MAX_N) return FAIL(SIGGAN_E_INVALID, "%s: n = %d outside [1, %d]", who, n, SIGGAN_KMEANS_MAX_N);
    if (dim < 1 || dim > SIGGAN_KMEANS_MAX_DIM) return FAIL(SIGGAN_E_INVALID, "%s: dim = %d outside [1, %d]", who, dim, SIGGAN_KMEANS_MAX_DIM);
    if (k < 1 || k > SIGGAN_KMEANS_MAX_K) return FAIL(SIGGAN_E_INVALID, "%s: k = %d outside [1, %d]", who, k, SIGGAN_KMEANS_MAX_K);
    if (k > n) return FAIL(SIGGAN_E_INVALID, "%s: k = %d exceeds the n = %d rows", who, k, n);
    const size_t need = layout(n).bytes;
    if (workspace_bytes < need)
        return FAIL(SIGGAN_E_INVALID, "%s: workspace of %zu bytes, %zu needed (siggan_kmeans_workspace)", who, workspace_bytes, need);
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return FAIL(SIGGAN_E_INVALID, "%s: workspace_dev must be 8-byte aligned", who);
    return SIGGAN_OK;
}

}  // namespace

extern "C" size_t siggan_kmeans_workspace(int32_t n, int32_t dim, int32_t k) {
    if (n < 1 || n > SIGGAN_KMEANS_MAX_N || dim < 1 || dim > SIGGAN_KMEANS_MAX_DIM || k < 1 || k > SIGGAN_KMEANS_MAX_K || k > n) return 0;
    return layout(n).bytes;
}

extern "C" int siggan_kmeans_seed(int32_t device, const float* x_dev, int32_t n, int32_t dim, int32_t k, uint64_t seed,
                                  float* centres_dev, int32_t* seed_rows_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!x_dev || !centres_dev || !seed_rows_dev || !workspace_dev) return FAIL(SIGGAN_E_INVALID, "siggan_kmeans_seed: null tensor");
    if (int rc = check_sizes("siggan_kmeans_seed", n, dim, k, workspace_dev, workspace_bytes)) return rc;
    DevGuard dg(device); HIPCHK(dg.err);
    const Layout l = layout(n);
    char* ws = static_cast<char*>(workspace_dev);
    double* m = reinterpret_cast<double*>(ws + l.v);
    double* sums = reinterpret_cast<double*>(ws + l.sums);
    const hipStream_t st = (hipStream_t)stream;
    for (int s = 0; s < k; ++s) {
        if (s) {
            hipLaunchKernelGGL(k_seed_update, dim3((unsigned)l.blocks), dim3(64 * WAVES), 0, st, x_dev, n, dim,
                               (const float*)(centres_dev + (size_t)(s - 1) * dim), s == 1 ? 1 : 0, m, sums);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_seed_pick, dim3(1), dim3(256), 0, st, x_dev, n, dim, s, (unsigned long long)seed, (const double*)m,
                           (const double*)sums, l.blocks, centres_dev, seed_rows_dev);
        HIPCHK(hipGetLastError());
    }
    return SIGGAN_OK;
}

extern "C" int siggan_kmeans_lloyd(int32_t device, const float* x_dev, int32_t n, int32_t dim, float* centres_dev, int32_t k,
                                   int32_t iterations, int32_t* label_dev, double* mind2_dev, int32_t* count_dev, double* inertia_dev,
                                   int32_t* changed_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!x_dev || !centres_dev || !label_dev || !count_dev || !inertia_dev || !changed_dev || !workspace_dev)
        return FAIL(SIGGAN_E_INVALID, "siggan_kmeans_lloyd: null tensor");
    if (int rc = check_sizes("siggan_kmeans_lloyd", n, dim, k, workspace_dev, workspace_bytes)) return rc;
    if (iterations < 0 || iterations > SIGGAN_KMEANS_MAX_ITERATIONS)
        return FAIL(SIGGAN_E_INVALID, "siggan_kmeans_lloyd: iterations = %d outside [0, %d]", iterations, SIGGAN_KMEANS_MAX_ITERATIONS);
    DevGuard dg(device); HIPCHK(dg.err);
    const Layout l = layout(n);
    char* ws = static_cast<char*>(workspace_dev);
    double* mind2 = mind2_dev ? mind2_dev : reinterpret_cast<double*>(ws + l.v);
    double* sums = reinterpret_cast<double*>(ws + l.sums);
    int32_t* prev = reinterpret_cast<int32_t*>(ws + l.prev);
    int32_t* part = reinterpret_cast<int32_t*>(ws + l.part);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned slabs = (unsigned)((dim + SLAB - 1) / SLAB);
    for (int t = 0; t <= iterations; ++t) {
        // the assignment IS siggan_knn with k = 1: the same kernel, hence the same bits
        if (int rc = siggan_knn(device, x_dev, n, centres_dev, k, dim, 1, 0, mind2, label_dev, stream)) return rc;
        hipLaunchKernelGGL(k_lloyd_stats, dim3((unsigned)l.blocks), dim3(64), 0, st, (const int32_t*)label_dev, (const double*)mind2, prev,
                           n, t == 0 ? 1 : 0, sums, part);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_lloyd_fold, dim3(1), dim3(256), 0, st, (const double*)sums, (const int32_t*)part, l.blocks, inertia_dev + t,
                           changed_dev + t);
        HIPCHK(hipGetLastError());
        const bool update = t < iterations;
        hipLaunchKernelGGL(k_lloyd_update, update ? dim3((unsigned)k, slabs) : dim3((unsigned)k), dim3(update ? SLAB : 64), 0, st, x_dev, n,
                           dim, (const int32_t*)label_dev, centres_dev, count_dev, update ? 1 : 0);
        HIPCHK(hipGetLastError());
    }
    return SIGGAN_OK;
}
