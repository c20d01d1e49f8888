// strokes_word_check.cpp -- a stand-alone host program (no device, not part of the library) that runs the word arithmetic
// of strokes_word.h the way k_strokes uses it -- one 64-bit word per "thread", two ping-pong buffers, one flag word per
// pass -- and compares it with a per-pixel restatement: thinning passes and skeleton, line ends and junction pixels, the
// distance map against brute force, the row dilation against a disc.  tests/test_strokes_cpu.py builds it with the host
// compiler under AddressSanitizer and UBSan and runs it.  Prints "OK <cases> cases, max passes <n>" and returns 0, or
// "FAIL ..." and 1.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#define SK_HD static inline
#include "strokes_word.h"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 11);
}

struct Image {
    int h, w;
    std::vector<uint8_t> m;
    int at(int y, int x) const { return (y < 0 || y >= h || x < 0 || x >= w) ? 0 : m[y * w + x]; }     // the paper goes on
};

// Guo-Hall A1 pixel by pixel -> passes, the one that deletes nothing included.
static int thin_per_pixel(Image& a) {
    for (int passes = 1;; ++passes) {
        bool changed = false;
        for (int sub = 0; sub < 2; ++sub) {
            Image b = a;
            for (int y = 0; y < a.h; ++y)
                for (int x = 0; x < a.w; ++x) {
                    if (!a.at(y, x)) continue;
                    const int P2 = a.at(y - 1, x), P3 = a.at(y - 1, x + 1), P4 = a.at(y, x + 1), P5 = a.at(y + 1, x + 1);
                    const int P6 = a.at(y + 1, x), P7 = a.at(y + 1, x - 1), P8 = a.at(y, x - 1), P9 = a.at(y - 1, x - 1);
                    const int C = ((1 - P2) & (P3 | P4)) + ((1 - P4) & (P5 | P6)) + ((1 - P6) & (P7 | P8)) + ((1 - P8) & (P9 | P2));
                    const int N = std::min((P9 | P2) + (P3 | P4) + (P5 | P6) + (P7 | P8), (P2 | P3) + (P4 | P5) + (P6 | P7) + (P8 | P9));
                    const int third = sub ? ((P6 | P7 | (1 - P9)) & P8) : ((P2 | P3 | (1 - P5)) & P4);
                    if (C == 1 && N >= 2 && N <= 3 && !third) { b.m[y * a.w + x] = 0; changed = true; }
                }
            a = b;
        }
        if (!changed) return passes;
    }
}

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf(" (case %d, %d x %d)\n", t, h, w); return 1; } } while (0)

int main() {
    static const int hs[] = {1, 2, 3, 5, 33, 64, 127, 128}, ws[] = {4, 8, 12, 64, 68, 124, 128};
    static const int radii2[] = {0, 1, 2, 4, 5, 8, 9, 16, 17, 25, 36};
    int max_passes = 0, t = 0, h = 0, w = 0;
    for (int d2 = 1; d2 <= 4096; ++d2) {
        const int k = sk_width_bin(d2);
        CHECK(k >= 1 && k <= 16 && (k == 16 || d2 <= k * k) && d2 > (k - 1) * (k - 1), "width bin of %d", d2);
    }
    for (t = 0; t < 300; ++t) {
        h = t ? hs[rnd() % 8] : 128;
        w = t ? ws[rnd() % 7] : 128;
        Image im{h, w, std::vector<uint8_t>((size_t)h * w)};
        const int mode = t % 4;                                          // sparse, half, dense noise; rectangles and holes
        const uint32_t dense = 900 + rnd() % 100;
        for (int i = 0; i < h * w; ++i) im.m[i] = (t == 0 || mode == 3) ? 1 : rnd() % 1000 < (mode == 0 ? 100u : mode == 1 ? 500u : dense);
        if (t && mode == 3)
            for (int k = 0; k < 6; ++k) {
                const int y0 = rnd() % h, x0 = rnd() % w, y1 = std::min(h, y0 + 1 + (int)(rnd() % 20)), x1 = std::min(w, x0 + 1 + (int)(rnd() % 20));
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) im.m[y * w + x] = k & 1;
            }

        // the kernel's thinning: 256 "threads", thread tid owns word tid & 1 of row tid >> 1
        std::vector<uint64_t> smask(2 * h, 0), bufb(2 * h, 0);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                if (im.m[y * w + x]) smask[2 * y + (x >> 6)] |= 1ull << (x & 63);
        std::vector<uint64_t> bufa = smask;
        const int nseg = (w + 63) >> 6, bound = std::max(h, w) + 2;
        std::vector<int> sflag(136, 0);
        int passes = -1;
        for (int pass = 1; pass <= bound; ++pass) {
            for (int sub = 0; sub < 2; ++sub) {
                std::vector<uint64_t>& from = sub ? bufb : bufa;
                std::vector<uint64_t>& to = sub ? bufa : bufb;
                for (int tid = 0; tid < 256; ++tid) {
                    if (!(tid < 2 * h && (tid & 1) < nseg)) continue;
                    const uint64_t p = from[tid];
                    const uint64_t del = p ? sk_deletions(p, sk_planes(from.data(), h, tid >> 1, tid & 1), sub) : 0;
                    to[tid] = p & ~del;
                    if (del) sflag.at(pass) = 1;
                }
            }
            if (!sflag[pass]) { passes = pass; break; }
        }
        Image sk = im;
        const int want_passes = thin_per_pixel(sk);
        CHECK(passes == want_passes, "passes %d, per pixel %d", passes, want_passes);
        max_passes = std::max(max_passes, passes);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < 128; ++x)
                CHECK((int)((bufa[2 * y + (x >> 6)] >> (x & 63)) & 1) == (x < w ? sk.m[y * w + x] : 0), "skeleton at (%d, %d)", y, x);

        // line ends and junction pixels
        int ends = 0, junctions = 0, want_ends = 0, want_junctions = 0;
        for (int tid = 0; tid < 2 * h; ++tid) {
            if (!bufa[tid]) continue;
            const SkPlanes n = sk_planes(bufa.data(), h, tid >> 1, tid & 1);
            ends += __builtin_popcountll(sk_endpoints(bufa[tid], n));
            junctions += __builtin_popcountll(sk_junctions(bufa[tid], n));
        }
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                if (!sk.at(y, x)) continue;
                const int ring[9] = {sk.at(y - 1, x), sk.at(y - 1, x + 1), sk.at(y, x + 1), sk.at(y + 1, x + 1), sk.at(y + 1, x),
                                     sk.at(y + 1, x - 1), sk.at(y, x - 1), sk.at(y - 1, x - 1), sk.at(y - 1, x)};
                int neighbours = 0, transitions = 0;
                for (int i = 0; i < 8; ++i) { neighbours += ring[i]; transitions += !ring[i] && ring[i + 1]; }
                want_ends += neighbours == 1;
                want_junctions += transitions >= 3;
            }
        CHECK(ends == want_ends && junctions == want_junctions, "ends %d / %d, junctions %d / %d", ends, want_ends, junctions, want_junctions);

        // distance map: the kernel's column scan and row search against brute force (quadratic: the smaller images and case 0)
        std::vector<uint8_t> g((size_t)h * w);
        for (int x = 0; x < w; ++x) {
            int d = 0;
            for (int y = 0; y < h; ++y) { d = im.m[y * w + x] ? d + 1 : 0; g[y * w + x] = (uint8_t)std::min(d, 255); }
            d = 0;
            for (int y = h - 1; y >= 0; --y) { d = im.m[y * w + x] ? d + 1 : 0; g[y * w + x] = (uint8_t)std::min(d, (int)g[y * w + x]); }
        }
        if (h * w <= 64 * 68 || t == 0) {
            std::vector<int> by, bx;
            for (int y = -1; y <= h; ++y)
                for (int x = -1; x <= w; ++x)
                    if (!im.at(y, x)) { by.push_back(y); bx.push_back(x); }
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    int want = 0;
                    if (im.m[y * w + x]) {
                        want = 1 << 30;
                        for (size_t k = 0; k < by.size(); ++k) want = std::min(want, (by[k] - y) * (by[k] - y) + (bx[k] - x) * (bx[k] - x));
                    }
                    const int got = im.m[y * w + x] ? sk_d2_row(g.data() + y * w, w, x) : 0;
                    CHECK(got == want && want <= 4096, "D2 %d, brute force %d at (%d, %d)", got, want, y, x);
                }
        }

        // the redraw's row masks against a disc
        const int r2 = radii2[rnd() % 11];
        for (int y = 0; y < h; ++y) {
            uint64_t lo, hi;
            sk_dilate_row(bufa.data(), h, w, y, r2, lo, hi);
            for (int x = 0; x < 128; ++x) {
                int want = 0;
                for (int dy = -6; dy <= 6 && x < w; ++dy)
                    for (int dx = -6; dx <= 6; ++dx) want |= dx * dx + dy * dy <= r2 && sk.at(y + dy, x + dx);
                CHECK((int)((x < 64 ? lo >> x : hi >> (x - 64)) & 1) == want, "dilation by %d at (%d, %d)", r2, y, x);
            }
        }
    }
    printf("OK %d cases, max passes %d\n", t, max_passes);
    return 0;
}
