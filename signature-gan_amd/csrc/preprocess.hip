// preprocess.hip -- scan preprocessing (include/siggan_preprocess.h): denoise, validate, crop, area resize, centre, CLAHE.
// gfx950 only.  Integers throughout but for the four doubles of the resize geometry; tests/preprocesscommon.py restates every
// stage in numpy and the kernels equal it exactly.
//
// k_pp_denoise: one workgroup per (scan, 64 x 64 output tile).  The grid is scans x (the largest tile count of a scan); a
//   workgroup whose tile number its scan does not have returns at once.  The tile of g with a halo of 3 up / left and 1
//   down / right is read into LDS with the blur's reflection (-1 -> 1, n -> n - 2) applied where the halo leaves the image;
//   b (66 x 66), e (65 x 65) and d (64 x 64) follow, each from LDS.  The tile's halo and the image's border are different
//   things: a position of b or e that is outside the IMAGE holds the neutral value of the stencil that reads it (255 for
//   the min, 0 for the max), which is what "skip" means; a position outside the TILE's halo is never read.  One WHITE
//   partial per tile goes to the workspace, so nothing needs zeroing and the sum has no order.
// k_pp_label: one workgroup of 1024 threads per scan, scratch in the workspace (a scan does not fit LDS).
//   1. a wave64 ballot of d <= 127 gives each row's ink mask, one word per 64 columns (bits at and beyond the width are 0);
//   2. a RUN is a maximal horizontal stretch of ink; two runs of a row cannot start in the same pair of columns, so
//      SLOT = y * ceil(w / 2) + (x >> 1) numbers them, and a smaller slot is an earlier run in raster order;
//   3. lab[slot] = slot; the thread that owns a run walks the part of the row above that the run touches (its columns
//      widened by one on each side: 8-connectivity) and joins itself with every run there.  The join is components.hip's
//      lock-free union-find on global memory: follow lab[] to both roots, point the larger at the smaller with an atomic
//      min, go on from the value it held if another thread got there first.  Links only ever point to smaller slots;
//   4. every run's link is replaced by its root and its length added to area[root] (integer atomic add);
//   5. components, kept components and the box of the kept ones are reduced with LDS atomic add / min / max.
//   Nothing iterates to a fixed point, yet every walk is bounded: a chain visits strictly decreasing slots (at most `nodes`
//   steps) and every retry of a join lowers one of its two roots (at most 2 * nodes retries).  A hit bound raises OVERFLOW.
// k_pp_finish<T>: one workgroup of 1024 threads per scan; the T x T canvas, sixteen histograms and the 64 LUTs live in LDS.
//   WHITE partials, crop geometry, box resample straight from the denoised pool, moments, shift, CLAHE, store.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/siggan_preprocess.h"
#include "host.h"
#include "preprocess_plan.h"

static_assert(PP_MIN_SIDE == SIGGAN_PP_MIN_SIDE && PP_MAX_SIDE == SIGGAN_PP_MAX_SIDE && PP_MAX_MARGIN == SIGGAN_PP_MAX_MARGIN &&
              PP_MAX_BATCH == SIGGAN_PP_MAX_BATCH, "preprocess_plan.h and siggan_preprocess.h state the same limits");

namespace {

constexpr int DN_THREADS = 256, LB_THREADS = 1024, FN_THREADS = 1024;
constexpr int INK_MAX = 127;                     // ink is byte <= 127, white is byte > 127
enum { BOX_COMPONENTS, BOX_KEPT, BOX_X0, BOX_Y0, BOX_X1, BOX_Y1, BOX_OVERFLOW };

struct Scan { int64_t off; int h, w, min_pixels; };
__device__ __forceinline__ Scan load_scan(const int64_t* __restrict__ geom, int img) {
    const int64_t* g = geom + 4 * (int64_t)img;
    return {g[0], (int)g[1], (int)g[2], (int)(g[3] > INT_MAX ? INT_MAX : g[3])};
}

// ---------------------------------------------------------------------------------------------------------- stage 1 and 2
__global__ __launch_bounds__(DN_THREADS) void k_pp_denoise(const uint8_t* __restrict__ pool, const int64_t* __restrict__ geom,
                                                           int max_tiles, int denoise, uint8_t* __restrict__ dpool,
                                                           int32_t* __restrict__ partials) {
    constexpr int TS = PP_TILE, GS = TS + 4, BS = TS + 2, ES = TS + 1;
    __shared__ uint8_t sg[GS][GS], sb[BS][GS], se[ES][GS];
    __shared__ int swhite;
    const int img = blockIdx.x / max_tiles, tile = blockIdx.x - img * max_tiles, tid = threadIdx.x;
    const Scan s = load_scan(geom, img);
    const int h = s.h, w = s.w, tiles_x = (w + TS - 1) / TS, tiles_y = (h + TS - 1) / TS;
    if (tile >= tiles_x * tiles_y) return;                               // block-uniform
    const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS;
    const uint8_t* src = pool + s.off;
    uint8_t* dst = dpool + s.off;
    if (tid == 0) swhite = 0;
    __syncthreads();
    int white = 0;
    if (!denoise) {
        for (int p = tid; p < TS * TS; p += DN_THREADS) {
            const int y = ty0 + (p >> 6), x = tx0 + (p & 63);
            if (y < h && x < w) {
                const int v = src[(size_t)y * w + x];
                dst[(size_t)y * w + x] = (uint8_t)v;
                white += v > INK_MAX;
            }
        }
    } else {
        for (int p = tid; p < GS * GS; p += DN_THREADS) {                // g, image rows ty0 - 3 .., columns tx0 - 3 ..
            const int i = p / GS, j = p - i * GS;
            int y = ty0 - 3 + i, x = tx0 - 3 + j;
            y = y == -1 ? 1 : (y == h ? h - 2 : y);                      // the blur's border; further out is never used
            x = x == -1 ? 1 : (x == w ? w - 2 : x);
            sg[i][j] = (y >= 0 && y < h && x >= 0 && x < w) ? src[(size_t)y * w + x] : (uint8_t)0;
        }
        __syncthreads();
        for (int p = tid; p < BS * BS; p += DN_THREADS) {                // b, image rows ty0 - 2 .., columns tx0 - 2 ..
            const int i = p / BS, j = p - i * BS, y = ty0 - 2 + i, x = tx0 - 2 + j;
            int v = 255;                                                 // outside the image: skipped by the min
            if (y >= 0 && y < h && x >= 0 && x < w) {
                const int r0 = sg[i][j] + 2 * sg[i][j + 1] + sg[i][j + 2];
                const int r1 = sg[i + 1][j] + 2 * sg[i + 1][j + 1] + sg[i + 1][j + 2];
                const int r2 = sg[i + 2][j] + 2 * sg[i + 2][j + 1] + sg[i + 2][j + 2];
                v = (r0 + 2 * r1 + r2 + 8) >> 4;
            }
            sb[i][j] = (uint8_t)v;
        }
        __syncthreads();
        for (int p = tid; p < ES * ES; p += DN_THREADS) {                // e, image rows ty0 - 1 .., columns tx0 - 1 ..
            const int i = p / ES, j = p - i * ES, y = ty0 - 1 + i, x = tx0 - 1 + j;
            int v = 0;                                                   // outside the image: skipped by the max
            if (y >= 0 && y < h && x >= 0 && x < w) v = min(min((int)sb[i][j + 1], (int)sb[i + 1][j]), (int)sb[i + 1][j + 1]);
            se[i][j] = (uint8_t)v;
        }
        __syncthreads();
        for (int p = tid; p < TS * TS; p += DN_THREADS) {
            const int i = p >> 6, j = p & 63, y = ty0 + i, x = tx0 + j;
            if (y < h && x < w) {
                const int v = max(max((int)se[i][j + 1], (int)se[i + 1][j]), (int)se[i + 1][j + 1]);
                dst[(size_t)y * w + x] = (uint8_t)v;
                white += v > INK_MAX;
            }
        }
    }
    if (white) atomicAdd(&swhite, white);
    __syncthreads();
    if (tid == 0) partials[(int64_t)img * PP_MAX_TILES + tile] = swhite;
}

// --------------------------------------------------------------------------------------------------------------- stage 3
// A row's mask: bit x & 63 of word x >> 6 for column x, nseg = ceil(w / 64) words, bits at and beyond the width 0.
__device__ __forceinline__ int row_bit(const uint64_t* row, int x) { return (int)(row[x >> 6] >> (x & 63)) & 1; }

// The end (exclusive) of the stretch of set bits that holds bit s.
__device__ __forceinline__ int run_end(const uint64_t* row, int s, int w, int nseg) {
    int idx = s >> 6;
    uint64_t v = ~row[idx] >> (s & 63);                                  // the zeros shifted in at the top are 0 here: not seen
    if (v) return min(s + __builtin_ctzll(v), w);
    for (++idx; idx < nseg; ++idx) {
        v = ~row[idx];
        if (v) return min(idx * 64 + __builtin_ctzll(v), w);
    }
    return w;
}

// The first bit of the stretch of set bits that holds bit b.
__device__ __forceinline__ int run_start(const uint64_t* row, int b) {
    int idx = b >> 6;
    const int sh = b & 63;
    uint64_t v = ~row[idx] & (sh == 63 ? ~0ull : ((1ull << (sh + 1)) - 1));   // the zeros below b
    for (;;) {
        if (v) return idx * 64 + 64 - __builtin_clzll(v);
        if (idx == 0) return 0;
        v = ~row[--idx];
    }
}

// The first set bit in [x, hi), hi <= w, or -1.
__device__ __forceinline__ int next_set(const uint64_t* row, int x, int hi) {
    while (x < hi) {
        const uint64_t v = row[x >> 6] >> (x & 63);
        if (v) {
            const int c = x + __builtin_ctzll(v);
            return c < hi ? c : -1;
        }
        x = ((x >> 6) + 1) << 6;
    }
    return -1;
}

// The first column of the run that starts in column pair k, or -1.
__device__ __forceinline__ int start_in_pair(const uint64_t* row, int k, int w) {
    const int x0 = 2 * k, x1 = x0 + 1;
    const int b0 = row_bit(row, x0), prev = x0 > 0 ? row_bit(row, x0 - 1) : 0, b1 = x1 < w ? row_bit(row, x1) : 0;
    return (b0 && !prev) ? x0 : ((b1 && !b0) ? x1 : -1);
}

__device__ __forceinline__ int load_lab(const int* lab, int x) { return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root of x's chain; sets bad when the chain is longer than any chain of strictly decreasing slots can be.
__device__ __forceinline__ int find_root(const int* lab, int x, int nodes, int& bad) {
    for (int steps = 0;; ++steps) {
        const int p = load_lab(lab, x);
        if (p == x) return x;
        if (steps >= nodes || p < 0 || p > x) { bad = 1; return x; }
        x = p;
    }
}

__device__ __forceinline__ void join(int* lab, int a, int b, int nodes, int& bad) {
    for (int tries = 0;; ++tries) {
        const int a0 = a, b0 = b;
        a = find_root(lab, a, nodes, bad);
        b = find_root(lab, b, nodes, bad);
        if (bad) return;
        // shorten the two chains just walked: the root found is an ancestor, and min keeps every link pointing downwards
        if (a != a0) atomicMin(lab + a0, a);
        if (b != b0) atomicMin(lab + b0, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                    // a > b: a is to point at b
        const int old = atomicMin(lab + a, b);
        if (old == a) return;                                            // a was still a root: linked
        if (tries >= 2 * nodes) { bad = 1; return; }
        a = old;                                                         // a had been re-pointed meanwhile: old < a, join it too
    }
}

__global__ __launch_bounds__(LB_THREADS) void k_pp_label(const uint8_t* __restrict__ dpool, const int64_t* __restrict__ geom,
                                                         uint64_t* masks_all, int* lab_all, int* area_all, int32_t* __restrict__ boxes) {
    __shared__ int sbox[PP_BOX_INTS];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Scan s = load_scan(geom, img);
    const int h = s.h, w = s.w, nseg = (w + 63) >> 6, wh = (w + 1) >> 1, nodes = h * wh;
    const uint8_t* d = dpool + s.off;
    uint64_t* masks = masks_all + ((s.off >> 6) + (int64_t)PP_SLACK * img);      // pp_mask_base
    int* lab = lab_all + ((s.off >> 1) + (int64_t)PP_SLACK * img);               // pp_slot_base
    int* area = area_all + ((s.off >> 1) + (int64_t)PP_SLACK * img);

    // 1. row masks, labels, areas
    if (tid < PP_BOX_INTS) sbox[tid] = (tid == BOX_X0 || tid == BOX_Y0) ? INT_MAX : ((tid == BOX_X1 || tid == BOX_Y1) ? -1 : 0);
    for (int item = wave; item < h * nseg; item += LB_THREADS / 64) {    // wave-uniform
        const int y = item / nseg, seg = item - y * nseg, x = seg * 64 + lane;
        const bool ink = x < w && (int)d[(size_t)y * w + x] <= INK_MAX;
        const uint64_t m = __ballot(ink);
        if (lane == 0) masks[item] = m;
    }
    for (int i = tid; i < nodes; i += LB_THREADS) { lab[i] = i; area[i] = 0; }
    __syncthreads();

    // 3. join every run with the runs it touches in the row above
    int bad = 0;
    for (int slot = wh + tid; slot < nodes && !bad; slot += LB_THREADS) {
        const int y = slot / wh, k = slot - y * wh;
        const uint64_t* row = masks + (size_t)y * nseg;
        const int st = start_in_pair(row, k, w);
        if (st < 0) continue;
        const int e = run_end(row, st, w, nseg);                         // the run is [st, e)
        const uint64_t* up = row - nseg;
        const int hi = min(e + 1, w);
        int x = max(st - 1, 0);
        while (!bad) {
            const int b = next_set(up, x, hi);
            if (b < 0) break;
            const int us = run_start(up, b), ue = run_end(up, b, w, nseg);       // the run above holding b is [us, ue)
            join(lab, slot, (y - 1) * wh + (us >> 1), nodes, bad);
            x = ue + 1;
        }
    }
    if (bad) sbox[BOX_OVERFLOW] = 1;
    __syncthreads();

    // 4. links to roots, areas.  The roots are final, so a stale link read by another thread still leads to the same root.
    bad = 0;
    for (int slot = tid; slot < nodes && !bad; slot += LB_THREADS) {
        const int y = slot / wh, k = slot - y * wh;
        const uint64_t* row = masks + (size_t)y * nseg;
        const int st = start_in_pair(row, k, w);
        if (st < 0) continue;
        const int len = run_end(row, st, w, nseg) - st;
        const int r = find_root(lab, slot, nodes, bad);
        if (r != slot) __hip_atomic_store(lab + slot, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        atomicAdd(area + r, len);
    }
    if (bad) sbox[BOX_OVERFLOW] = 1;
    __syncthreads();

    // 5. components, kept components, the box of the kept ones
    int comps = 0, kept = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    if (!sbox[BOX_OVERFLOW]) {
        for (int slot = tid; slot < nodes; slot += LB_THREADS) {
            const int y = slot / wh, k = slot - y * wh;
            const uint64_t* row = masks + (size_t)y * nseg;
            const int st = start_in_pair(row, k, w);
            if (st < 0) continue;
            const int e = run_end(row, st, w, nseg);
            const int r = load_lab(lab, slot);
            const int a = __hip_atomic_load(area + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (r == slot) { ++comps; kept += a >= s.min_pixels; }
            if (a >= s.min_pixels) { x0 = min(x0, st); x1 = max(x1, e - 1); y0 = min(y0, y); y1 = max(y1, y); }
        }
    }
    if (comps) { atomicAdd(&sbox[BOX_COMPONENTS], comps); if (kept) atomicAdd(&sbox[BOX_KEPT], kept); }
    if (x1 >= 0) {
        atomicMin(&sbox[BOX_X0], x0); atomicMin(&sbox[BOX_Y0], y0);
        atomicMax(&sbox[BOX_X1], x1); atomicMax(&sbox[BOX_Y1], y1);
    }
    __syncthreads();
    if (tid < PP_BOX_INTS) boxes[(int64_t)img * PP_BOX_INTS + tid] = sbox[tid];
}

// ----------------------------------------------------------------------------------------------------------- stages 4 to 6
// round-half-even of num / den, num >= 0, den > 0
__device__ __forceinline__ int div_rhe(int num, int den) {
    const int q = num / den, r = num - q * den;
    return q + ((2 * r > den || (2 * r == den && (q & 1))) ? 1 : 0);
}

struct FinishOptions { int crop, center, equalize, margin; };
enum { F_CX, F_CY, F_CW, F_CH, F_NW, F_NH, F_DEGENERATE, F_SX, F_SY, F_COUNT };

template <int T>
__global__ __launch_bounds__(FN_THREADS) void k_pp_finish(const uint8_t* __restrict__ dpool, const int64_t* __restrict__ geom,
                                                          const int32_t* __restrict__ partials, const int32_t* __restrict__ boxes,
                                                          FinishOptions opt, uint8_t* __restrict__ out, int32_t* __restrict__ stats,
                                                          uint8_t* __restrict__ canvas_out) {
    constexpr int GRID = 8, TILE = T / GRID, AREA = TILE * TILE, CLIP = (2 * AREA / 256) > 1 ? (2 * AREA / 256) : 1;
    constexpr int WAVES = FN_THREADS / 64;
    __shared__ uint8_t sc[T * T];                                        // the canvas before the shift
    __shared__ uint8_t slut[GRID * GRID][256];
    __shared__ int shist[WAVES][256];
    __shared__ int sstat[SIGGAN_PP_COUNT];
    __shared__ int sf[F_COUNT];
    __shared__ int smom[3];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Scan s = load_scan(geom, img);
    const int h = s.h, w = s.w;
    const uint8_t* d = dpool + s.off;
    uint8_t* o = out + (size_t)img * T * T;
    uint8_t* co = canvas_out ? canvas_out + (size_t)img * T * T : nullptr;

    if (tid < SIGGAN_PP_COUNT) sstat[tid] = 0;
    if (tid < 3) smom[tid] = 0;
    __syncthreads();
    const int tiles = ((h + PP_TILE - 1) / PP_TILE) * ((w + PP_TILE - 1) / PP_TILE);
    if (tid < tiles) atomicAdd(&sstat[SIGGAN_PP_WHITE], partials[(int64_t)img * PP_MAX_TILES + tid]);
    if (tid == 0) {
        int status = 0, cx = 0, cy = 0, cw = w, ch = h;
        if (opt.crop) {
            const int32_t* b = boxes + (int64_t)img * PP_BOX_INTS;
            if (b[BOX_OVERFLOW]) status |= SIGGAN_PP_OVERFLOW;
            else {
                sstat[SIGGAN_PP_COMPONENTS] = b[BOX_COMPONENTS];
                sstat[SIGGAN_PP_KEPT] = b[BOX_KEPT];
            }
            if (b[BOX_OVERFLOW] || b[BOX_KEPT] < 1) status |= SIGGAN_PP_NO_BBOX;
            else {
                const int bw = b[BOX_X1] - b[BOX_X0] + 1, bh = b[BOX_Y1] - b[BOX_Y0] + 1;
                cx = max(0, b[BOX_X0] - opt.margin);
                cy = max(0, b[BOX_Y0] - opt.margin);
                cw = min(w - cx, bw + 2 * opt.margin);
                ch = min(h - cy, bh + 2 * opt.margin);
            }
        }
        const double sx = (double)T / (double)cw, sy = (double)T / (double)ch;
        const double scale = sy < sx ? sy : sx;                          // Python's min(T / cw, T / ch)
        int nw = (int)((double)cw * scale), nh = (int)((double)ch * scale);
        const int degenerate = nw < 1 || nh < 1;
        if (degenerate) { status |= SIGGAN_PP_DEGENERATE; nw = 0; nh = 0; }
        nw = min(nw, T); nh = min(nh, T);                                // cannot bind: cw * scale <= T up to one rounding, which int() absorbs
        sstat[SIGGAN_PP_STATUS] = status;
        sstat[SIGGAN_PP_CROP_X] = cx; sstat[SIGGAN_PP_CROP_Y] = cy; sstat[SIGGAN_PP_CROP_W] = cw; sstat[SIGGAN_PP_CROP_H] = ch;
        sstat[SIGGAN_PP_NEW_W] = nw; sstat[SIGGAN_PP_NEW_H] = nh;
        sf[F_CX] = cx; sf[F_CY] = cy; sf[F_CW] = cw; sf[F_CH] = ch; sf[F_NW] = nw; sf[F_NH] = nh; sf[F_DEGENERATE] = degenerate;
        sf[F_SX] = 0; sf[F_SY] = 0;
    }
    __syncthreads();
    if (sf[F_DEGENERATE]) {                                              // block-uniform
        for (int p = tid; p < T * T; p += FN_THREADS) { o[p] = 255; if (co) co[p] = 255; }
        if (tid < SIGGAN_PP_COUNT) stats[(int64_t)img * SIGGAN_PP_COUNT + tid] = sstat[tid];
        return;
    }

    // 4. the exact box average of the crop, pasted on paper
    {
        const int cx = sf[F_CX], cy = sf[F_CY], cw = sf[F_CW], ch = sf[F_CH], nw = sf[F_NW], nh = sf[F_NH];
        const int xo = (T - nw) / 2, yo = (T - nh) / 2, den = cw * ch;
        for (int p = tid; p < T * T; p += FN_THREADS) {
            const int Y = p / T - yo, X = p % T - xo;
            int v = 255;
            if (Y >= 0 && Y < nh && X >= 0 && X < nw) {
                const int xa = X * cw, xb = xa + cw, ya = Y * ch, yb = ya + ch;  // the output pixel, in units of 1 / nw and 1 / nh of a source pixel
                const int x_lo = xa / nw, x_hi = (xb + nw - 1) / nw, y_lo = ya / nh, y_hi = (yb + nh - 1) / nh;
                int acc = 0;
                for (int y = y_lo; y < y_hi; ++y) {
                    const int oy = min((y + 1) * nh, yb) - max(y * nh, ya);
                    const uint8_t* row = d + (size_t)(cy + y) * w + cx;
                    int rs = 0;
                    for (int x = x_lo; x < x_hi; ++x) rs += (min((x + 1) * nw, xb) - max(x * nw, xa)) * (int)row[x];
                    acc += oy * rs;
                }
                v = (acc + (den >> 1)) / den;
            }
            sc[p] = (uint8_t)v;
        }
    }
    __syncthreads();

    // 5. moments of 255 - canvas and the whole-pixel shift
    if (opt.center) {
        int m00 = 0, m10 = 0, m01 = 0;
        for (int p = tid; p < T * T; p += FN_THREADS) {
            const int v = 255 - (int)sc[p];
            m00 += v; m10 += (p % T) * v; m01 += (p / T) * v;
        }
        if (m00) { atomicAdd(&smom[0], m00); atomicAdd(&smom[1], m10); atomicAdd(&smom[2], m01); }
        __syncthreads();
        if (tid == 0) {
            sstat[SIGGAN_PP_M00] = smom[0];
            if (smom[0] > 0) {
                sf[F_SX] = T / 2 - smom[1] / smom[0];
                sf[F_SY] = T / 2 - smom[2] / smom[0];
                sstat[SIGGAN_PP_SHIFT_X] = sf[F_SX]; sstat[SIGGAN_PP_SHIFT_Y] = sf[F_SY];
            }
        }
        __syncthreads();
    }
    const int shx = sf[F_SX], shy = sf[F_SY];
    auto centred = [&](int y, int x) -> int {                            // the canvas after the shift
        const int yy = y - shy, xx = x - shx;
        return (yy >= 0 && yy < T && xx >= 0 && xx < T) ? (int)sc[yy * T + xx] : 255;
    };
    if (co) for (int p = tid; p < T * T; p += FN_THREADS) co[p] = (uint8_t)centred(p / T, p % T);
    if (tid < SIGGAN_PP_COUNT) stats[(int64_t)img * SIGGAN_PP_COUNT + tid] = sstat[tid];
    if (!opt.equalize) {                                                 // block-uniform
        for (int p = tid; p < T * T; p += FN_THREADS) o[p] = (uint8_t)centred(p / T, p % T);
        return;
    }

    // 6. CLAHE: one wave per tile, sixteen tiles at a time; a lane owns four neighbouring bins
    for (int round = 0; round < GRID * GRID / WAVES; ++round) {
        const int tile = round * WAVES + wave, ty = tile / GRID, tx = tile - ty * GRID;
        for (int j = 0; j < 4; ++j) shist[wave][4 * lane + j] = 0;
        __syncthreads();
        for (int p = lane; p < AREA; p += 64) atomicAdd(&shist[wave][centred(ty * TILE + p / TILE, tx * TILE + p % TILE)], 1);
        __syncthreads();
        int hb[4], excess = 0;
        for (int j = 0; j < 4; ++j) {
            hb[j] = shist[wave][4 * lane + j];
            excess += max(hb[j] - CLIP, 0);
            hb[j] = min(hb[j], CLIP);
        }
        for (int off = 32; off > 0; off >>= 1) excess += __shfl_xor(excess, off, 64);
        const int batch = excess >> 8, residual = excess & 255, step = residual > 0 ? max(256 / residual, 1) : 1;
        int sum = 0;
        for (int j = 0; j < 4; ++j) {
            const int bin = 4 * lane + j;
            hb[j] += batch + ((residual > 0 && bin % step == 0 && bin / step < residual) ? 1 : 0);
            sum += hb[j];
        }
        int incl = sum;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        int cum = incl - sum;
        for (int j = 0; j < 4; ++j) {
            cum += hb[j];
            slut[tile][4 * lane + j] = (uint8_t)min(div_rhe(cum * 255, AREA), 255);
        }
        __syncthreads();
    }
    for (int p = tid; p < T * T; p += FN_THREADS) {
        const int y = p / T, x = p % T, v = centred(y, x);
        const int ny = 2 * y - TILE, nx = 2 * x - TILE;                  // (y / TILE - 0.5) and (x / TILE - 0.5) in units of 1 / (2 TILE)
        const int ty1 = ny < 0 ? -1 : ny / (2 * TILE), tx1 = nx < 0 ? -1 : nx / (2 * TILE);
        const int ya = ny - ty1 * 2 * TILE, xa = nx - tx1 * 2 * TILE, yb = 2 * TILE - ya, xb = 2 * TILE - xa;
        const int r1 = max(ty1, 0), r2 = min(ty1 + 1, GRID - 1), c1 = max(tx1, 0), c2 = min(tx1 + 1, GRID - 1);
        const int top = (int)slut[r1 * GRID + c1][v] * xb + (int)slut[r1 * GRID + c2][v] * xa;
        const int bot = (int)slut[r2 * GRID + c1][v] * xb + (int)slut[r2 * GRID + c2][v] * xa;
        o[p] = (uint8_t)div_rhe(top * yb + bot * ya, 4 * AREA);
    }
}

}  // namespace

extern "C" size_t siggan_preprocess_workspace(int64_t total_pixels, int32_t n) {
    if (n < 1 || n > SIGGAN_PP_MAX_BATCH || total_pixels < 1) return 0;
    return pp_layout(total_pixels, n).bytes;
}

extern "C" int siggan_preprocess_u8(int32_t device, const uint8_t* pool_dev, int64_t total_pixels, const int64_t* geom_host,
                                    const int64_t* geom_dev, int32_t n, const siggan_preprocess_options* options, uint8_t* out_dev,
                                    int32_t* stats_dev, uint8_t* denoised_dev, uint8_t* canvas_dev, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    if (n < 1 || n > SIGGAN_PP_MAX_BATCH) return FAIL(SIGGAN_E_INVALID, "n = %d outside [1, %d]", n, SIGGAN_PP_MAX_BATCH);
    if (!pool_dev) return FAIL(SIGGAN_E_INVALID, "null pool_dev");
    if (!geom_host || !geom_dev) return FAIL(SIGGAN_E_INVALID, "null geometry table: give geom_host and geom_dev");
    if (!options) return FAIL(SIGGAN_E_INVALID, "null options");
    if (!out_dev) return FAIL(SIGGAN_E_INVALID, "missing out_dev");
    if (!stats_dev) return FAIL(SIGGAN_E_INVALID, "missing stats_dev");
    if (!workspace_dev) return FAIL(SIGGAN_E_INVALID, "null workspace_dev");
    if (options->target != 64 && options->target != 128) return FAIL(SIGGAN_E_INVALID, "target must be 64 or 128, got %d", options->target);
    if (options->margin < 0 || options->margin > SIGGAN_PP_MAX_MARGIN)
        return FAIL(SIGGAN_E_INVALID, "margin = %d outside [0, %d]", options->margin, SIGGAN_PP_MAX_MARGIN);
    if (total_pixels < 1) return FAIL(SIGGAN_E_INVALID, "total_pixels = %lld < 1", (long long)total_pixels);
    int64_t at = 0;
    int max_tiles = 0;
    const PpGeomError ge = pp_check_geometry(geom_host, n, total_pixels, &at, &max_tiles);
    const long long i = (long long)at, off = (long long)geom_host[4 * at], gh = (long long)geom_host[4 * at + 1],
                    gw = (long long)geom_host[4 * at + 2], mp = (long long)geom_host[4 * at + 3];
    switch (ge) {
        case PP_GEOM_OK: break;
        case PP_GEOM_HEIGHT: return FAIL(SIGGAN_E_INVALID, "scan %lld: height = %lld outside [%d, %d]", i, gh, SIGGAN_PP_MIN_SIDE, SIGGAN_PP_MAX_SIDE);
        case PP_GEOM_WIDTH: return FAIL(SIGGAN_E_INVALID, "scan %lld: width = %lld outside [%d, %d]", i, gw, SIGGAN_PP_MIN_SIDE, SIGGAN_PP_MAX_SIDE);
        case PP_GEOM_MIN_PIXELS: return FAIL(SIGGAN_E_INVALID, "scan %lld: min_pixels = %lld < 1", i, mp);
        case PP_GEOM_OFFSET_NEGATIVE: return FAIL(SIGGAN_E_INVALID, "scan %lld: offset = %lld < 0", i, off);
        case PP_GEOM_OFFSET_ORDER: return FAIL(SIGGAN_E_INVALID, "scan %lld: offset = %lld overlaps the scan before it (offsets ascend)", i, off);
        case PP_GEOM_OFFSET_PAST_END:
            return FAIL(SIGGAN_E_INVALID, "scan %lld: offset = %lld + %lld x %lld runs past total_pixels = %lld", i, off, gh, gw, (long long)total_pixels);
    }
    const PpLayout L = pp_layout(total_pixels, n);
    if (workspace_bytes < L.bytes) return FAIL(SIGGAN_E_INVALID, "workspace of %zu bytes is too small: %zu needed", workspace_bytes, L.bytes);
    if (reinterpret_cast<uintptr_t>(workspace_dev) & 7) return FAIL(SIGGAN_E_INVALID, "workspace_dev must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(stats_dev) & 3) || (reinterpret_cast<uintptr_t>(geom_dev) & 7))
        return FAIL(SIGGAN_E_INVALID, "stats_dev must be 4-byte aligned and geom_dev 8-byte aligned");

    unsigned char* ws = static_cast<unsigned char*>(workspace_dev);
    uint8_t* dpool = denoised_dev ? denoised_dev : ws + L.pool;
    int32_t* partials = reinterpret_cast<int32_t*>(ws + L.partials);
    int32_t* boxes = reinterpret_cast<int32_t*>(ws + L.boxes);
    hipStream_t st = (hipStream_t)stream;
    DevGuard dg(device); HIPCHK(dg.err);
    hipLaunchKernelGGL(k_pp_denoise, dim3((unsigned)((int64_t)n * max_tiles)), dim3(DN_THREADS), 0, st, pool_dev, geom_dev, max_tiles,
                       options->denoise ? 1 : 0, dpool, partials);
    HIPCHK(hipGetLastError());
    if (options->crop) {
        hipLaunchKernelGGL(k_pp_label, dim3((unsigned)n), dim3(LB_THREADS), 0, st, dpool, geom_dev, reinterpret_cast<uint64_t*>(ws + L.masks),
                           reinterpret_cast<int*>(ws + L.lab), reinterpret_cast<int*>(ws + L.area), boxes);
        HIPCHK(hipGetLastError());
    }
    const FinishOptions fo = {options->crop ? 1 : 0, options->center ? 1 : 0, options->equalize ? 1 : 0, options->margin};
    if (options->target == 64)
        hipLaunchKernelGGL(k_pp_finish<64>, dim3((unsigned)n), dim3(FN_THREADS), 0, st, dpool, geom_dev, partials, boxes, fo, out_dev, stats_dev, canvas_dev);
    else
        hipLaunchKernelGGL(k_pp_finish<128>, dim3((unsigned)n), dim3(FN_THREADS), 0, st, dpool, geom_dev, partials, boxes, fo, out_dev, stats_dev, canvas_dev);
    HIPCHK(hipGetLastError());
    return SIGGAN_OK;
}
