// warp_plan_check.cpp -- a stand-alone host program (no device, not part of the library) that holds warp_plan.h to what the
// kernel of warp.hip needs, over every height 1..128, every width 4..128 that is a multiple of 4 and every cell: the control
// grid covers every tap of every pixel, the drawing threads fit one workgroup and their groups the control region, the LDS
// parts are aligned, disjoint and inside 64 KiB; and per cell: the weights are non-negative and sum to 6 c^3 at every
// offset, the amplitude bound is floor(0.4 c 256) and lies under the control bound, a horizontal sum of the largest control
// values fits int32, and wp_round equals floor((2 S + den) / (2 den)) on exact, half-way and extreme sums of both signs.
// tests/test_warp_cpu.py builds it with the host compiler under AddressSanitizer and UBSan and runs it.  Prints
// "OK <cases>" and returns 0, or "FAIL ..." and 1.
#include <stdio.h>

#include "warp_plan.h"

static int fail(const char* what, long long a, long long b, long long c) {
    printf("FAIL %s: %lld, %lld, %lld\n", what, a, b, c);
    return 1;
}

// floor division of 128-bit-safe operands: 2 S + den stays below 2^51
static int64_t floordiv(int64_t a, int64_t b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

int main() {
    long cases = 0;
    const int cells[] = {8, 16, 32};
    for (int c : cells) {
        if (!wp_cell_ok(c) || (1 << wp_log2(c)) != c) return fail("cell", c, wp_log2(c), 0);
        if (wp_max_amp(c) != (int)(0.4 * c * 256) || wp_max_amp(c) > WP_MAX_CTRL) return fail("amplitude bound", c, wp_max_amp(c), 0);
        const int64_t sum = 6 * (int64_t)c * c * c;
        for (int k = 0; k < c; ++k) {
            int64_t s = 0;
            for (int b = 0; b < 4; ++b) {
                if (wp_weight(b, k, c) < 0) return fail("negative weight", c, k, b);
                s += wp_weight(b, k, c);
            }
            if (s != sum) return fail("weights do not sum to 6 c^3", c, k, s);
            ++cases;
        }
        if (sum * WP_MAX_CTRL > INT32_MAX) return fail("horizontal sum leaves int32", c, sum, 0);
        const int64_t den = wp_den(c), top = sum * sum * WP_MAX_CTRL;             // |S| <= top
        if (den != sum * sum || (INT64_C(36) << (6 * wp_log2(c))) != den) return fail("den", c, den, 0);
        // exact multiples, the half-way points on both sides, the extremes, and a seeded sweep
        uint64_t state = 0x9e3779b97f4a7c15ull + (uint64_t)c;
        for (int t = 0; t < 200000; ++t) {
            int64_t S;
            if (t < 20000) {
                const int64_t d = (t / 4) - 2500;                                    // displacement -2500 .. 2499
                const int64_t off[4] = {0, den / 2 - 1, den / 2, -(den / 2) - 1};   // 2 S + den even: S = d den +- den / 2 are the ties
                S = d * den + off[t % 4];
            } else if (t < 20004) {
                const int64_t ends[4] = {top, -top, top - 1, -top + 1};
                S = ends[t - 20000];
            } else {
                state = state * 6364136223846793005ull + 1442695040888963407ull;
                S = (int64_t)((state >> 13) % (uint64_t)(2 * top + 1)) - top;
            }
            const int64_t want = floordiv(2 * S + den, 2 * den);
            if (wp_round(S, wp_log2(c)) != want) return fail("wp_round", c, S, want);
            if (want > WP_MAX_CTRL || want < -WP_MAX_CTRL) return fail("disp beyond the control bound", c, S, want);
            ++cases;
        }
        for (int h = 1; h <= WP_MAX_SIZE; ++h)
            for (int w = 4; w <= WP_MAX_SIZE; w += 4, ++cases) {
                const int gx = wp_grid(w, c), gy = wp_grid(h, c);
                if ((w - 1) / c + 3 > gx - 1 || (h - 1) / c + 3 > gy - 1) return fail("a tap past the grid", h, w, c);
                if (gx != (w + c - 1) / c + 3 || gy != (h + c - 1) / c + 3) return fail("grid extents", h, w, c);
                if (wp_groups(h, w, c) > WP_THREADS || 4 * wp_groups(h, w, c) < wp_elements(h, w, c)) return fail("drawing threads", h, w, c);
                const WpLayout L = wp_layout(h, w, c);
                if (L.image != 0 || L.ctrl < h * w || L.ctrl % 16 || L.hsum < L.ctrl + 4 * wp_elements(h, w, c) || L.hsum % 16 ||
                    L.hsum != L.ctrl + 16 * wp_groups(h, w, c) || L.bytes != L.hsum + 8 * gy * w || L.bytes > 65536)
                    return fail("LDS layout", h, w, c);
            }
    }
    printf("OK %ld\n", cases);
    return 0;
}
