// strokes_word.h -- the arithmetic of strokes.hip that works on whole 64-bit words of row masks, and the row search of the
// distance map.  Plain integer functions of their arguments: they compile for the host too (define SK_HD empty), which is how
// they are checked against a per-pixel restatement without a device.
//
// A row mask is two 64-bit words (bit x & 63 of word x >> 6 is column x); bits at and beyond the image width are 0 and stay
// 0, and rows outside the image read as 0: "the paper goes on".
#pragma once
#include <stdint.h>

#ifndef SK_HD
#define SK_HD __host__ __device__ __forceinline__
#endif

// The eight neighbour planes of word s of row y, named as in include/siggan_strokes.h: bit x of p4 is pixel (x + 1, y), ...
struct SkPlanes {
    uint64_t p2, p3, p4, p5, p6, p7, p8, p9;
};

// Word s of a row shifted by one column with the carry between the row's two words: bit x is the row's bit x - 1 / x + 1.
SK_HD uint64_t sk_from_west(uint64_t lo, uint64_t hi, int s) { return s ? (hi << 1) | (lo >> 63) : lo << 1; }
SK_HD uint64_t sk_from_east(uint64_t lo, uint64_t hi, int s) { return s ? hi >> 1 : (lo >> 1) | (hi << 63); }

SK_HD SkPlanes sk_planes(const uint64_t* m, int h, int y, int s) {
    const uint64_t nlo = y > 0 ? m[2 * (y - 1)] : 0, nhi = y > 0 ? m[2 * (y - 1) + 1] : 0;
    const uint64_t slo = y + 1 < h ? m[2 * (y + 1)] : 0, shi = y + 1 < h ? m[2 * (y + 1) + 1] : 0;
    const uint64_t clo = m[2 * y], chi = m[2 * y + 1];
    SkPlanes n;
    n.p2 = s ? nhi : nlo;
    n.p3 = sk_from_east(nlo, nhi, s);
    n.p4 = sk_from_east(clo, chi, s);
    n.p5 = sk_from_east(slo, shi, s);
    n.p6 = s ? shi : slo;
    n.p7 = sk_from_west(slo, shi, s);
    n.p8 = sk_from_west(clo, chi, s);
    n.p9 = sk_from_west(nlo, nhi, s);
    return n;
}

// Of four one-bit planes: exactly one set / at least two set / all four set.
SK_HD uint64_t sk_one_of4(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return ((a ^ b) ^ (c ^ d)) & ~(a & b) & ~(c & d); }
SK_HD uint64_t sk_two_of4(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return (a & b) | (c & d) | ((a ^ b) & (c ^ d)); }
SK_HD uint64_t sk_all_of4(uint64_t a, uint64_t b, uint64_t c, uint64_t d) { return a & b & c & d; }

// The pixels of word p that sub-iteration `sub` (0 or 1) of a Guo-Hall pass deletes.  min(N1, N2) is 2 or 3 iff both are at
// least 2 and not both are 4.
SK_HD uint64_t sk_deletions(uint64_t p, const SkPlanes& n, int sub) {
    const uint64_t c1 = sk_one_of4(~n.p2 & (n.p3 | n.p4), ~n.p4 & (n.p5 | n.p6), ~n.p6 & (n.p7 | n.p8), ~n.p8 & (n.p9 | n.p2));
    const uint64_t a1 = n.p9 | n.p2, a2 = n.p3 | n.p4, a3 = n.p5 | n.p6, a4 = n.p7 | n.p8;
    const uint64_t b1 = n.p2 | n.p3, b2 = n.p4 | n.p5, b3 = n.p6 | n.p7, b4 = n.p8 | n.p9;
    const uint64_t n23 = sk_two_of4(a1, a2, a3, a4) & sk_two_of4(b1, b2, b3, b4) & ~(sk_all_of4(a1, a2, a3, a4) & sk_all_of4(b1, b2, b3, b4));
    const uint64_t third = sub ? (n.p6 | n.p7 | ~n.p9) & n.p8 : (n.p2 | n.p3 | ~n.p5) & n.p4;
    return p & c1 & n23 & ~third;
}

// Adds the one-bit plane v to the bit-sliced counters b0 (ones) .. b3 (eights), one counter per pixel of the word.
SK_HD void sk_count(uint64_t v, uint64_t& b0, uint64_t& b1, uint64_t& b2, uint64_t& b3) {
    const uint64_t c0 = b0 & v;
    b0 ^= v;
    const uint64_t c1 = b1 & c0;
    b1 ^= c0;
    const uint64_t c2 = b2 & c1;
    b2 ^= c1;
    b3 ^= c2;
}

// Pixels of skeleton word p with exactly one 8-neighbour on the skeleton.
SK_HD uint64_t sk_endpoints(uint64_t p, const SkPlanes& n) {
    uint64_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    sk_count(n.p2, b0, b1, b2, b3); sk_count(n.p3, b0, b1, b2, b3); sk_count(n.p4, b0, b1, b2, b3); sk_count(n.p5, b0, b1, b2, b3);
    sk_count(n.p6, b0, b1, b2, b3); sk_count(n.p7, b0, b1, b2, b3); sk_count(n.p8, b0, b1, b2, b3); sk_count(n.p9, b0, b1, b2, b3);
    return p & b0 & ~b1 & ~b2 & ~b3;
}

// Pixels of skeleton word p with three or more 0 -> 1 transitions around the ring P2, P3, ..., P9, P2 (there are at most 4).
SK_HD uint64_t sk_junctions(uint64_t p, const SkPlanes& n) {
    uint64_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    sk_count(~n.p2 & n.p3, b0, b1, b2, b3); sk_count(~n.p3 & n.p4, b0, b1, b2, b3); sk_count(~n.p4 & n.p5, b0, b1, b2, b3);
    sk_count(~n.p5 & n.p6, b0, b1, b2, b3); sk_count(~n.p6 & n.p7, b0, b1, b2, b3); sk_count(~n.p7 & n.p8, b0, b1, b2, b3);
    sk_count(~n.p8 & n.p9, b0, b1, b2, b3); sk_count(~n.p9 & n.p2, b0, b1, b2, b3);
    return p & ((b0 & b1) | b2 | b3);
}

// D2 of column x of a row whose column distances are g[0..w) (0 on background; the columns outside the image are background,
// so g is 0 there): the minimum over x' of (x - x')^2 + g[x']^2.  A column dx away cannot improve a minimum <= dx^2, so the
// search ends there and is still exact.
SK_HD int sk_d2_row(const uint8_t* g, int w, int x) {
    const int own = g[x];
    int best = own * own;
    for (int dx = 1; dx * dx < best; ++dx) {
        const int gl = x - dx >= 0 ? g[x - dx] : 0, gr = x + dx < w ? g[x + dx] : 0;
        const int gm = gl < gr ? gl : gr;
        const int cand = dx * dx + gm * gm;
        best = cand < best ? cand : best;
    }
    return best;
}

// Row y of the disc dilation of the masks m (h rows) by squared radius radius2 <= 36, clipped to w columns: the OR over
// |dy| <= 6 of row y + dy shifted by every dx with dx^2 + dy^2 <= radius2.
SK_HD void sk_dilate_row(const uint64_t* m, int h, int w, int y, int radius2, uint64_t& lo, uint64_t& hi) {
    typedef unsigned __int128 u128;
    u128 acc = 0;
    for (int dy = -6; dy <= 6; ++dy) {
        const int yy = y + dy, rem = radius2 - dy * dy;
        if (yy < 0 || yy >= h || rem < 0) continue;
        const u128 r = (u128)m[2 * yy] | ((u128)m[2 * yy + 1] << 64);
        if (!r) continue;
        u128 d = r;
        for (int dx = 1; dx * dx <= rem; ++dx) d |= (r << dx) | (r >> dx);
        acc |= d;
    }
    if (w < 128) acc &= ((u128)1 << w) - 1;
    lo = (uint64_t)acc;
    hi = (uint64_t)(acc >> 64);
}

// The width bin k in 1..16 of a skeleton pixel: the smallest k with D2 <= k^2, 16 for everything above 15^2.  d2 >= 1.
SK_HD int sk_width_bin(int d2) {
    int k = 1;
    while (k < 16 && d2 > k * k) ++k;
    return k;
}
