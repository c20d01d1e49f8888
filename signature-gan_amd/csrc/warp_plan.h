// warp_plan.h -- the host side of siggan_warp_u8's geometry and integer ranges: grid extents, the LDS layout per
// (h, w, cell), the amplitude bound, the B-spline weights and the rounding of the weighted sum.  No HIP in it: it compiles
// with -x c++, which is how warp_plan_check.cpp holds it to what the kernel of warp.hip needs over every allowed
// (h, w, cell).  Everything is constexpr, so the kernel calls the same functions.
//
// Ranges.  |D| <= WP_MAX_CTRL = 2^13 and the weights of one axis are >= 0 and sum to 6 c^3 <= 6 * 2^15, so a horizontal sum
// is at most 6 * 2^28 < 2^31: int32.  S, the vertical sum of those, is at most 36 c^6 * 2^13 <= 36 * 2^43 < 2^49: int64.
// disp = floor((2 S + den) / (2 den)) with den = 36 c^6 = 36 * 2^(6 l), l = log2 c.  2 den = 9 * 2^(6 l + 3), and for floor
// division floor(floor(a / m) / n) = floor(a / (m n)), so disp = floor(((2 S + den) >> (6 l + 3)) / 9) with an arithmetic
// shift: the shifted value is below 9 * 2^13 + 5 in magnitude, and the division by 9 is a 32-bit one.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int WP_MAX_SIZE = 128, WP_THREADS = 256, WP_PARAMS = 12, WP_MAX_N = 1 << 20;
constexpr int WP_MAX_CTRL = 8192;

constexpr bool wp_cell_ok(int c) { return c == 8 || c == 16 || c == 32; }
constexpr int wp_log2(int c) { return c == 8 ? 3 : c == 16 ? 4 : 5; }
constexpr int wp_max_amp(int c) { return c * 512 / 5; }                       // floor(0.4 * c * 256)
constexpr int wp_grid(int extent, int c) { return (extent + c - 1) / c + 3; }   // control points along an axis
constexpr int wp_elements(int h, int w, int c) { return 2 * wp_grid(h, c) * wp_grid(w, c); }
constexpr int wp_groups(int h, int w, int c) { return (wp_elements(h, w, c) + 3) / 4; }   // Philox groups = drawing threads

// LDS: the image (bytes, padded to 16), the control points (int32, whole groups), the horizontal sums (int32 [2][gy][w])
struct WpLayout { int image, ctrl, hsum, bytes; };
constexpr WpLayout wp_layout(int h, int w, int c) {
    const int image_bytes = (h * w + 15) & ~15;
    const int ctrl_bytes = 16 * wp_groups(h, w, c);
    const int hsum_bytes = 4 * 2 * wp_grid(h, c) * w;
    return WpLayout{0, image_bytes, image_bytes + ctrl_bytes, image_bytes + ctrl_bytes + hsum_bytes};
}

// weight b of offset k in a cell of c pixels; the four sum to 6 c^3
constexpr int32_t wp_weight(int b, int k, int c) {
    return b == 0 ? (c - k) * (c - k) * (c - k)
         : b == 1 ? 3 * k * k * k - 6 * c * k * k + 4 * c * c * c
         : b == 2 ? -3 * k * k * k + 3 * c * k * k + 3 * c * c * k + c * c * c
                  : k * k * k;
}
constexpr int64_t wp_den(int c) { return 36 * (int64_t)c * c * c * c * c * c; }
constexpr int32_t wp_floordiv9(int32_t t) { return t >= 0 ? t / 9 : -((8 - t) / 9); }
// floor((2 S + den) / (2 den)) by one shift and one 32-bit division (see above)
constexpr int32_t wp_round(int64_t S, int log2c) {
    return wp_floordiv9((int32_t)((2 * S + (INT64_C(36) << (6 * log2c))) >> (6 * log2c + 3)));
}
