// components.hip -- connected-component labelling of byte images (include/siggan_components.h).  gfx950 only.
//
// k_components: one workgroup of eight waves per image; the image, the row masks and the labels live in LDS
// (height * 16 + 3 * height * width bytes: 50 KiB at 128 x 128, three workgroups per CU).
//   1. the image is copied to LDS a word at a time; a wave64 ballot of byte < threshold gives each row's ink mask, one
//      64-bit word per 64 columns.  The kernel is instantiated over the mask type: uint64_t for widths up to 64, a 128-bit
//      pair beyond (bits at and beyond the width are 0);
//   2. a RUN is a maximal stretch of set bits; its first bit is a bit of m & ~(m << 1).  Two runs of a row cannot start in
//      the same pair of columns, so (row, start column / 2) numbers the runs: SLOT = y * (width / 2) + (x >> 1), at most
//      height * width / 2 = 8192 of them, and a smaller slot is an earlier run in raster order;
//   3. lab[slot] = slot; then the thread that owns a run walks the part of the row above that the run touches (its own
//      columns, widened by one on each side under 8-connectivity) and joins itself with every run found there.  The join is
//      a lock-free union-find: follow lab[] to both roots, point the larger root at the smaller with an LDS atomic min, and
//      if the atomic finds that the larger one had already been re-pointed by another thread, go on from the value it held.
//      The two slots a join started from are re-pointed at the roots it found (atomic min again), which keeps chains short.
//      Links only ever point to smaller slots, so there are no cycles and the root of a component is its smallest slot --
//      its first run -- whatever the order of the joins;
//   4. in one more pass every run's link is replaced by its root and its length is added to the HIGH half of lab[root]
//      with an LDS atomic add (slots take 13 bits, areas at most 15), so labels and areas share one word;
//   5. the counters are reduced per thread and then with LDS atomic add / min / max; root map and cleaned copy are written
//      with one pixel / one word per thread.
// Nothing iterates to a fixed point.  Still, every walk is bounded: a chain visits strictly decreasing slots (at most
// `nodes` steps) and every retry of a join lowers one of its two roots (at most 2 * nodes retries).  A thread that exceeds
// either raises a flag; the image then gets COMPONENTS = -1 and no other output.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/siggan_components.h"
#include "host.h"
#include "ink_rows.h"

namespace {

typedef unsigned __int128 u128;
constexpr int THREADS = 512;

// A row's ink mask is one 64-bit word for widths up to 64 and a 128-bit pair beyond; the kernel is written once over M.
__device__ __forceinline__ int ctz(uint64_t v) { return v ? __builtin_ctzll(v) : 64; }                  // bits of M for v == 0
__device__ __forceinline__ int ctz(u128 v) {
    const uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);
    return lo ? __builtin_ctzll(lo) : (hi ? 64 + __builtin_ctzll(hi) : 128);
}
__device__ __forceinline__ int top(uint64_t v) { return 63 - __builtin_clzll(v); }                     // highest set bit, v != 0
__device__ __forceinline__ int top(u128 v) {
    const uint64_t lo = (uint64_t)v, hi = (uint64_t)(v >> 64);
    return hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo);
}
template <typename M> __device__ __forceinline__ M below(int n) {                                      // bits [0, n), n >= 0
    return n >= (int)(8 * sizeof(M)) ? ~(M)0 : (M)(((M)1 << n) - 1);
}
template <typename M> __device__ __forceinline__ M row_mask(const uint64_t* smask, int y);
template <> __device__ __forceinline__ uint64_t row_mask<uint64_t>(const uint64_t* smask, int y) { return smask[2 * y]; }
template <> __device__ __forceinline__ u128 row_mask<u128>(const uint64_t* smask, int y) { return (u128)smask[2 * y] | ((u128)smask[2 * y + 1] << 64); }
template <typename M> __device__ __forceinline__ M run_starts(M m) { return m & ~(m << 1); }
// The end (exclusive) of the stretch of set bits of m that holds bit s; a stretch that reaches M's last bit ends at w.
template <typename M> __device__ __forceinline__ int run_end(M m, int s, int w) { return min(s + ctz((M)(~m >> s)), w); }
// The first column of the run that starts in column pair k of a row whose run starts are `starts`, or -1.
template <typename M> __device__ __forceinline__ int start_in_pair(M starts, int k) {
    const int two = (int)(starts >> (2 * k)) & 3;
    return two ? 2 * k + ((two & 1) ? 0 : 1) : -1;
}

__device__ __forceinline__ int load_lab(const int* lab, int x) { return __atomic_load_n(lab + x, __ATOMIC_RELAXED); }

// The root of x's chain; sets bad when the chain is longer than any chain of strictly decreasing slots can be.
__device__ __forceinline__ int find_root(const int* lab, int x, int nodes, int& bad) {
    for (int steps = 0;; ++steps) {
        const int p = load_lab(lab, x) & 0xffff;                         // (the high half holds an area once phase 4 runs)
        if (p == x) return x;
        if (steps >= nodes) { bad = 1; return x; }
        x = p;
    }
}

__device__ __forceinline__ void join(int* lab, int a, int b, int nodes, int& bad) {
    for (int tries = 0;; ++tries) {
        const int a0 = a, b0 = b;
        a = find_root(lab, a, nodes, bad);
        b = find_root(lab, b, nodes, bad);
        // shorten the two chains just walked: the root found is an ancestor, and min keeps every link pointing downwards
        if (a != a0) atomicMin(lab + a0, a);
        if (b != b0) atomicMin(lab + b0, b);
        if (a == b || bad) return;
        if (a < b) { const int t = a; a = b; b = t; }                    // a > b: a is to point at b
        const int old = atomicMin(lab + a, b);
        if (old == a) return;                                            // a was still a root: linked
        if (tries >= 2 * nodes) { bad = 1; return; }
        a = old;                                                         // a had been re-pointed meanwhile: old < a, join it too
    }
}

template <int CONN, typename M>
__global__ __launch_bounds__(THREADS) void k_components(const uint8_t* u8, int h, int w, int thr, int min_area, int fill,
                                                        int32_t* __restrict__ stats, int32_t* __restrict__ root, uint8_t* clean) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int sstat[SIGGAN_CC_COUNT + 1];                           // the counters and the bound flag
    const int hw = h * w, wh = w >> 1, nodes = h * wh, words = hw >> 2;
    uint64_t* smask = reinterpret_cast<uint64_t*>(smem);                 // h x 2
    int* lab = reinterpret_cast<int*>(smem + 16 * h);                    // nodes
    unsigned* simg32 = reinterpret_cast<unsigned*>(smem + 16 * h + 4 * nodes);   // words
    const uint8_t* simg = reinterpret_cast<const uint8_t*>(simg32);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t img = blockIdx.x;
    constexpr int C8 = CONN == 8 ? 1 : 0;

    // 1. image and row masks
    const unsigned* g32 = reinterpret_cast<const unsigned*>(u8 + img * hw);
    for (int i = tid; i < words; i += THREADS) simg32[i] = g32[i];
    for (int i = tid; i < 2 * h; i += THREADS) smask[i] = 0;
    for (int i = tid; i < nodes; i += THREADS) lab[i] = i;
    if (tid <= SIGGAN_CC_COUNT) sstat[tid] = (tid == SIGGAN_CC_X0 || tid == SIGGAN_CC_Y0) ? INT_MAX : (tid >= SIGGAN_CC_X1 && tid <= SIGGAN_CC_Y1 ? -1 : 0);
    __syncthreads();
    const int nseg = (w + 63) >> 6;
    for (int item = wave; item < h * nseg; item += THREADS / 64) {
        const int y = item / nseg, seg = item - y * nseg;
        const uint64_t m = ink_word(simg, w, y, seg, lane, thr);
        if (lane == 0) smask[2 * y + seg] = m;
    }
    __syncthreads();

    // 3. join every run with the runs it touches in the row above
    int bad = 0;
    for (RowWalk t(wh + tid, THREADS, wh); t.i < nodes && !bad; t.next()) {       // slot t.i = (row t.y, column pair t.x)
        const M m = row_mask<M>(smask, t.y);
        const int s = start_in_pair(run_starts(m), t.x);
        if (s < 0) continue;
        const int e = run_end(m, s, w);                                  // the run is [s, e)
        const M up = row_mask<M>(smask, t.y - 1), ups = run_starts(up);
        M touch = up & below<M>(e + C8) & ~below<M>(s - C8 > 0 ? s - C8 : 0);
        while (touch && !bad) {
            const int b = ctz(touch);
            const int us = top((M)(ups & below<M>(b + 1))), ue = run_end(up, b, w);   // the run above holding b is [us, ue)
            join(lab, t.i, (t.y - 1) * wh + (us >> 1), nodes, bad);
            touch &= ~below<M>(ue);
        }
    }
    if (bad) sstat[SIGGAN_CC_COUNT] = 1;
    __syncthreads();

    // 4. links to roots and areas in one pass.  The roots are final, so a stale link read by another thread still leads to
    //    the same root; the run lengths go into the high half of the root's word, which find_root masks off, and the word
    //    of a run that is no root only ever holds its link.
    bad = 0;
    int ink = 0;
    for (RowWalk t(tid, THREADS, wh); t.i < nodes && !bad; t.next()) {
        const M m = row_mask<M>(smask, t.y);
        const int s = start_in_pair(run_starts(m), t.x);
        if (s < 0) continue;
        const int len = run_end(m, s, w) - s;
        const int r = find_root(lab, t.i, nodes, bad);
        if (r != t.i) __atomic_store_n(lab + t.i, r, __ATOMIC_RELAXED);
        ink += len;
        atomicAdd(lab + r, len << 16);
    }
    if (bad) sstat[SIGGAN_CC_COUNT] = 1;
    __syncthreads();
    if (sstat[SIGGAN_CC_COUNT]) {                                        // block-uniform
        if (stats && tid < SIGGAN_CC_COUNT) stats[img * SIGGAN_CC_COUNT + tid] = tid == SIGGAN_CC_COMPONENTS ? -1 : 0;
        return;
    }

    // 5. counters
    if (stats) {
        int comps = 0, largest = 0, small = 0, small_ink = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
        for (RowWalk t(tid, THREADS, wh); t.i < nodes; t.next()) {
            const int slot = t.i, y = t.y;
            const M m = row_mask<M>(smask, y);
            const int s = start_in_pair(run_starts(m), t.x);
            if (s < 0) continue;
            const int e = run_end(m, s, w);
            const int r = lab[slot] & 0xffff, area = lab[r] >> 16;
            if (r == slot) {
                ++comps;
                largest = max(largest, area);
                if (area < min_area) { ++small; small_ink += area; }
            }
            if (area >= min_area) { x0 = min(x0, s); x1 = max(x1, e - 1); y0 = min(y0, y); y1 = max(y1, y); }
        }
        if (ink) atomicAdd(&sstat[SIGGAN_CC_INK], ink);
        if (comps) {
            atomicAdd(&sstat[SIGGAN_CC_COMPONENTS], comps);
            atomicMax(&sstat[SIGGAN_CC_LARGEST], largest);
            if (small) { atomicAdd(&sstat[SIGGAN_CC_SMALL_COMPONENTS], small); atomicAdd(&sstat[SIGGAN_CC_SMALL_INK], small_ink); }
        }
        if (x1 >= 0) {
            atomicMin(&sstat[SIGGAN_CC_X0], x0); atomicMin(&sstat[SIGGAN_CC_Y0], y0);
            atomicMax(&sstat[SIGGAN_CC_X1], x1); atomicMax(&sstat[SIGGAN_CC_Y1], y1);
        }
        __syncthreads();
        if (tid < SIGGAN_CC_COUNT) {
            int v = sstat[tid];
            if (tid >= SIGGAN_CC_X0 && sstat[SIGGAN_CC_X1] < 0) v = -1;
            stats[img * SIGGAN_CC_COUNT + tid] = v;
        }
    }

    //    root map: one pixel per thread
    if (root) {
        int32_t* out = root + img * hw;
        for (int p = tid; p < hw; p += THREADS) {
            const int y = p / w, x = p - y * w;
            const M m = row_mask<M>(smask, y);
            int v = -1;
            if ((int)(m >> x) & 1) {
                const int us = top((M)(run_starts(m) & below<M>(x + 1)));
                const int r = lab[y * wh + (us >> 1)] & 0xffff;
                const int ry = r / wh;
                v = ry * w + start_in_pair(run_starts(row_mask<M>(smask, ry)), r - ry * wh);
            }
            out[p] = v;
        }
    }

    //    cleaned copy: one word (four pixels of one row) per thread; in place, only changed words are stored
    if (clean) {
        unsigned* out = reinterpret_cast<unsigned*>(clean + img * hw);
        const bool in_place = clean == u8;
        for (int i = tid; i < words; i += THREADS) {
            const int p = i << 2, y = p / w, x = p - y * w;
            const M m = row_mask<M>(smask, y);
            const unsigned v = simg32[i];
            unsigned o = v;
            const int four = (int)(m >> x) & 15;
            if (four) {
                const M starts = run_starts(m);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((four >> j) & 1) {
                        const int us = top((M)(starts & below<M>(x + j + 1)));
                        const int area = lab[lab[y * wh + (us >> 1)] & 0xffff] >> 16;
                        if (area < min_area) o = (o & ~(255u << (8 * j))) | ((unsigned)fill << (8 * j));
                    }
            }
            if (!in_place || o != v) out[i] = o;
        }
    }
}

}  // namespace

extern "C" int siggan_components_u8(int32_t device, const uint8_t* u8_dev, int32_t batch, int32_t height, int32_t width,
                                    int32_t threshold, int32_t connectivity, int32_t min_area, int32_t fill,
                                    int32_t* stats_dev, int32_t* root_dev, uint8_t* clean_dev, void* stream) {
    const char* no_output = !stats_dev && !root_dev && !clean_dev ? "no output: give stats_dev, root_dev or clean_dev" : nullptr;
    if (int rc = ink_refuse_images(u8_dev, no_output, batch, height, width, SIGGAN_CC_MAX_SIZE, threshold)) return rc;
    if (connectivity != 4 && connectivity != 8) return FAIL(SIGGAN_E_INVALID, "connectivity must be 4 or 8, got %d", connectivity);
    if (min_area < 1) return FAIL(SIGGAN_E_INVALID, "min_area = %d < 1", min_area);
    if (int rc = ink_refuse_fill(fill, threshold, "a cleaned pixel must not be ink")) return rc;
    if (int rc = ink_refuse_unaligned({u8_dev, stats_dev, root_dev, clean_dev}, "u8_dev, stats_dev, root_dev and clean_dev")) return rc;
    const size_t lds = (size_t)16 * height + (size_t)3 * height * width;     // masks + labels (2 B per pixel) + image
    DevGuard dg(device); HIPCHK(dg.err);
    void (*kernel)(const uint8_t*, int, int, int, int, int, int32_t*, int32_t*, uint8_t*) =
        width <= 64 ? (connectivity == 8 ? k_components<8, uint64_t> : k_components<4, uint64_t>)
                    : (connectivity == 8 ? k_components<8, u128> : k_components<4, u128>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)batch), dim3(THREADS), lds, (hipStream_t)stream, u8_dev, height, width, threshold, min_area,
                       fill, stats_dev, root_dev, clean_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
