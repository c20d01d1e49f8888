// strokes.hip -- stroke geometry of byte images (include/siggan_strokes.h): distance map, Guo-Hall skeleton, counters, redraw.
// gfx950 only.
//
// k_strokes: one workgroup of four waves per image; everything lives in dynamic LDS (48 * height + 640 bytes, plus
// height * width when the distance map is needed: 23 168 bytes at 128 x 128).
//   1. a wave64 ballot of byte < threshold gives each row's ink mask, two 64-bit words per row as in k_components (bits at
//      and beyond the width are 0).  This is the only read of the image, so redraw_dev may be u8_dev;
//   2. thinning on whole words (strokes_word.h): thread t owns word t & 1 of row t >> 1 -- 2 * height <= 256 words, one per
//      thread -- and decides its 64 pixels per sub-iteration from the eight neighbour planes.  Two ping-pong buffers: the first
//      sub-iteration reads A and writes B, the second reads B and writes A, a barrier after each.
//      THE LOOP'S EXIT IS UNIFORM: pass p has a flag word of its own, sflag[p], zeroed before the first barrier of the kernel,
//      raised (LDS atomic max) only by deletions of pass p, i.e. only before the second barrier of pass p, and read by every
//      thread only after that barrier.  No thread writes sflag[p] again, so all threads read the same value, leave the loop
//      in the same pass and have met the same number of barriers.  The loop is bounded by max(height, width) + 2 passes
//      (full rectangles need at most max / 2 + 2); an image that reaches the bound gets PASSES = -1 and no other output;
//   3. endpoints and junction pixels come out of the same planes with bit-sliced counters; ink and skeleton are popcounts;
//   4. g(x, y), the distance to the nearest background pixel of the column, one thread per column (a byte per pixel); then
//      every ink pixel searches its row for the minimum of dx^2 + g^2, ending at dx^2 >= the minimum so far.  D2 is consumed
//      where it is computed (global store, maximum, histogram of the skeleton's pixels) and never stored in LDS;
//   5. the redraw ORs shifted skeleton rows into one 128-bit mask per row (buffer B is free by then); skeleton and redraw
//      are written one word (four pixels of one row) per thread.
// Integers only; LDS atomic add and max do not depend on order.  No global atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/siggan_strokes.h"
#include "host.h"
#include "ink_rows.h"
#include "strokes_word.h"

namespace {

constexpr int THREADS = 256;                                            // = 2 * SIGGAN_SK_MAX_SIZE: one mask word per thread
constexpr int FLAGS = 136;                                               // sflag[1 .. max + 2], rounded up to 16 bytes
constexpr int STATS = 24;                                                // SIGGAN_SK_COUNT rounded up likewise
static_assert(THREADS == 2 * SIGGAN_SK_MAX_SIZE && FLAGS > SIGGAN_SK_MAX_SIZE + 2 && STATS >= SIGGAN_SK_COUNT && FLAGS % 4 == 0 && STATS % 4 == 0, "");

__host__ __device__ constexpr size_t lds_bytes(int h, int w, bool distance) {
    return (size_t)48 * h + 4 * (FLAGS + STATS) + (distance ? (size_t)h * w : 0);
}

// Four bits (0/1 bytes of one word) times v: bit j -> byte j.
__device__ __forceinline__ unsigned spread4(int four) { return (four & 1) | ((four & 2) << 7) | ((four & 4) << 14) | ((four & 8) << 21); }

__global__ __launch_bounds__(THREADS) void k_strokes(const uint8_t* u8, int h, int w, int thr, int radius2, int ink, int fill,
                                                     int32_t* __restrict__ stats, int16_t* __restrict__ d2out, uint8_t* __restrict__ skel,
                                                     uint8_t* redraw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* smask = reinterpret_cast<uint64_t*>(smem);                 // h x 2: the ink
    uint64_t* bufa = smask + 2 * h;                                      // h x 2: the thinning state, then the skeleton
    uint64_t* bufb = bufa + 2 * h;                                       // h x 2: the other state, then the redraw's mask
    int* sflag = reinterpret_cast<int*>(bufb + 2 * h);                   // FLAGS
    int* sstat = sflag + FLAGS;                                          // STATS
    uint8_t* g = reinterpret_cast<uint8_t*>(sstat + STATS);              // h x w, only with stats or d2out
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hw = h * w, words = hw >> 2, nseg = (w + 63) >> 6;
    const size_t img = blockIdx.x;
    const bool distance = stats || d2out;

    // 1. row masks
    const uint8_t* src = u8 + img * hw;
    for (int item = wave; item < 2 * h; item += THREADS / 64) {          // wave-uniform
        const uint64_t m = ink_word(src, w, item >> 1, item & 1, lane, thr);
        if (lane == 0) { smask[item] = m; bufa[item] = m; bufb[item] = 0; }
    }
    for (int i = tid; i < FLAGS + STATS; i += THREADS) sflag[i] = 0;     // (sstat follows sflag)
    __syncthreads();

    // 2. thinning
    const bool mine = tid < 2 * h && (tid & 1) < nseg;
    const int my_y = tid >> 1, my_s = tid & 1;
    const int bound = max(h, w) + 2;
    int passes = -1;
    for (int pass = 1; pass <= bound; ++pass) {
        if (mine) {
            const uint64_t p = bufa[tid];
            const uint64_t del = p ? sk_deletions(p, sk_planes(bufa, h, my_y, my_s), 0) : 0;
            bufb[tid] = p & ~del;
            if (del) atomicMax(&sflag[pass], 1);
        }
        __syncthreads();
        if (mine) {
            const uint64_t p = bufb[tid];
            const uint64_t del = p ? sk_deletions(p, sk_planes(bufb, h, my_y, my_s), 1) : 0;
            bufa[tid] = p & ~del;
            if (del) atomicMax(&sflag[pass], 1);
        }
        __syncthreads();
        if (sflag[pass] == 0) { passes = pass; break; }                  // block-uniform: see the head of the file
    }
    if (passes < 0) {                                                    // block-uniform
        if (stats && tid < SIGGAN_SK_COUNT) stats[img * SIGGAN_SK_COUNT + tid] = tid == SIGGAN_SK_PASSES ? -1 : 0;
        return;
    }

    // 3. counters of the masks; 4. column distances
    if (stats && mine) {
        const uint64_t p = bufa[tid];
        const int n_ink = __builtin_popcountll(smask[tid]);
        if (n_ink) atomicAdd(&sstat[SIGGAN_SK_INK], n_ink);
        if (p) {
            const SkPlanes n = sk_planes(bufa, h, my_y, my_s);
            const int ends = __builtin_popcountll(sk_endpoints(p, n)), junctions = __builtin_popcountll(sk_junctions(p, n));
            atomicAdd(&sstat[SIGGAN_SK_SKELETON], __builtin_popcountll(p));
            if (ends) atomicAdd(&sstat[SIGGAN_SK_ENDPOINTS], ends);
            if (junctions) atomicAdd(&sstat[SIGGAN_SK_JUNCTION_PIXELS], junctions);
        }
    }
    if (distance) {
        if (tid < w) {
            int d = 0;                                                   // the row above the image is background
            for (int y = 0; y < h; ++y) {
                d = bit_at(smask, y, tid) ? d + 1 : 0;
                g[y * w + tid] = (uint8_t)min(d, 255);                   // (the upward scan brings it to at most (h + 1) / 2)
            }
            d = 0;
            for (int y = h - 1; y >= 0; --y) {
                d = bit_at(smask, y, tid) ? d + 1 : 0;
                g[y * w + tid] = (uint8_t)min(d, (int)g[y * w + tid]);
            }
        }
        __syncthreads();
        int d2_max = 0, d2_sum = 0;
        int16_t* out = d2out ? d2out + img * hw : nullptr;
        for (int p = tid, y = tid / w, x = tid % w; p < hw; p += THREADS) {
            const int d2 = bit_at(smask, y, x) ? sk_d2_row(g + y * w, w, x) : 0;
            if (out) out[p] = (int16_t)d2;
            d2_max = max(d2_max, d2);
            if (stats && d2 && bit_at(bufa, y, x)) {
                d2_sum += d2;
                atomicAdd(&sstat[SIGGAN_SK_WIDTH_HIST + sk_width_bin(d2) - 1], 1);
            }
            x += THREADS % w; y += THREADS / w;
            if (x >= w) { x -= w; ++y; }
        }
        if (stats) {
            if (d2_max) atomicMax(&sstat[SIGGAN_SK_D2_MAX], d2_max);
            if (d2_sum) atomicAdd(&sstat[SIGGAN_SK_D2_SKEL_SUM], d2_sum);
        }
    }
    if (stats) {
        __syncthreads();
        if (tid < SIGGAN_SK_COUNT) stats[img * SIGGAN_SK_COUNT + tid] = tid == SIGGAN_SK_PASSES ? passes : sstat[tid];
    }

    // 5. skeleton and redraw: one word (four pixels of one row, inside one mask word) per thread
    if (skel) {
        unsigned* out = reinterpret_cast<unsigned*>(skel + img * hw);
        for (int i = tid, y = (4 * tid) / w, x = (4 * tid) % w; i < words; i += THREADS) {
            out[i] = spread4((int)(bufa[2 * y + (x >> 6)] >> (x & 63)) & 15);
            x += (4 * THREADS) % w; y += (4 * THREADS) / w;
            if (x >= w) { x -= w; ++y; }
        }
    }
    if (redraw) {
        if (tid < h) sk_dilate_row(bufa, h, w, tid, radius2, bufb[2 * tid], bufb[2 * tid + 1]);      // the disc, row by row
        __syncthreads();
        unsigned* out = reinterpret_cast<unsigned*>(redraw + img * hw);
        const unsigned base = 0x01010101u * (unsigned)fill, delta = (unsigned)(ink ^ fill);
        for (int i = tid, y = (4 * tid) / w, x = (4 * tid) % w; i < words; i += THREADS) {
            out[i] = base ^ (spread4((int)(bufb[2 * y + (x >> 6)] >> (x & 63)) & 15) * delta);
            x += (4 * THREADS) % w; y += (4 * THREADS) / w;
            if (x >= w) { x -= w; ++y; }
        }
    }
}

}  // namespace

extern "C" int siggan_strokes_u8(int32_t device, const uint8_t* u8_dev, int32_t batch, int32_t height, int32_t width,
                                 int32_t threshold, int32_t radius2, int32_t ink, int32_t fill,
                                 int32_t* stats_dev, int16_t* d2_dev, uint8_t* skel_dev, uint8_t* redraw_dev, void* stream) {
    const char* no_output = !stats_dev && !d2_dev && !skel_dev && !redraw_dev ? "no output: give stats_dev, d2_dev, skel_dev or redraw_dev" : nullptr;
    if (int rc = ink_refuse_images(u8_dev, no_output, batch, height, width, SIGGAN_SK_MAX_SIZE, threshold)) return rc;
    if (radius2 < 0 || radius2 > SIGGAN_SK_MAX_RADIUS2) return FAIL(SIGGAN_E_INVALID, "radius2 = %d outside [0, %d]", radius2, SIGGAN_SK_MAX_RADIUS2);
    if (ink < 0 || ink >= threshold)
        return FAIL(SIGGAN_E_INVALID, "ink = %d outside [0, threshold - 1 = %d]: a redrawn stroke must be ink", ink, threshold - 1);
    if (int rc = ink_refuse_fill(fill, threshold, "the paper must not be ink")) return rc;
    if (int rc = ink_refuse_unaligned({u8_dev, stats_dev, skel_dev, redraw_dev}, "u8_dev, stats_dev, skel_dev and redraw_dev")) return rc;
    if (reinterpret_cast<uintptr_t>(d2_dev) & 1) return FAIL(SIGGAN_E_INVALID, "d2_dev must be 2-byte aligned");
    DevGuard dg(device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_strokes, dim3((unsigned)batch), dim3(THREADS), lds_bytes(height, width, stats_dev || d2_dev), (hipStream_t)stream,
                       u8_dev, height, width, threshold, radius2, ink, fill, stats_dev, d2_dev, skel_dev, redraw_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
