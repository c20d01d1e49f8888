/*
 * siggan_warp.h -- C ABI of the signature duplicator on the MI355X: smooth random warps of byte images.  One real signature
 * in, many plausible same-writer variants out, by a free-form cubic B-spline deformation (the idea of Diaz et al.'s
 * duplicator) on top of an affine base map.  It needs no network weights.
 *
 * Definition (exact, integers only).  Images are uint8 (n, h, w), 1 <= h <= 128, w a multiple of 4 in 4..128.  Output image
 * i is the warp of source image index[i] (clamped into 0..n_src - 1; a null index means i).  Positions are Q8, 1/256 pixel;
 * a pixel index is the pixel's centre.
 *
 *   Control grid.  cell c in {8, 16, 32}; gx = ceil(w / c) + 3 columns and gy = ceil(h / c) + 3 rows; control point (j, i)
 *   -- row j, column i -- sits at pixel ((i - 1) c, (j - 1) c) and holds a displacement D[comp][j][i] in Q8, comp 0 = x,
 *   comp 1 = y.
 *
 *   Draws.  Image i has a 64-bit draw id d in its parameter row, so its result does not depend on its place in the batch.
 *   Element e = (comp * gy + j) * gx + i is word e & 3 of draw_raw(seed, ctr = d, idx = e >> 2, SIGGAN_WARP_STREAM)
 *   (csrc/rng.h); s = (int32)(word >> 16) - 32768; D = (s * amp[comp]) >> 15, an arithmetic shift, so |D| <= amp.  amp_x,
 *   amp_y are the image's amplitudes in Q8, 0 <= amp <= SIGGAN_WARP_MAX_AMP(c) = floor(0.4 * c * 256): 0.4 cells is the
 *   known sufficient bound for an injective cubic B-spline deformation (Choi & Lee 2000).  The rows live on the device, so
 *   the call cannot refuse a larger amplitude: the caller checks it, and the kernel clamps amp into that range.
 *   With ctrl_dev (int16 [n][2][gy][gx]) given, D is read from it instead, clamped into +-SIGGAN_WARP_MAX_CTRL, and nothing
 *   is drawn; whether such a field folds is the caller's business.
 *
 *   Interpolation.  Uniform cubic B-spline with integer weights: for k = x mod c (y mod c for the rows)
 *       B0 = (c - k)^3    B1 = 3k^3 - 6ck^2 + 4c^3    B2 = -3k^3 + 3ck^2 + 3c^2 k + c^3    B3 = k^3       (sum 6c^3)
 *   and with cx = x / c, cy = y / c (integer division)
 *       S    = sum_b B_b(y mod c) * sum_a B_a(x mod c) * D[comp][cy + b][cx + a]                  (exact, int64)
 *       disp = floor((2 S + den) / (2 den)),  den = 36 c^6                   (one rounding, half up, floor division)
 *   so |disp| <= max |D|.
 *
 *   Base map.  A per-image affine in 16.16: base = ((a2 + y a1 + x a0) >> 8, (a5 + y a4 + x a3) >> 8) in Q8, formed
 *   without wrapping (64-bit), the shift arithmetic.  Identity is a0 = a4 = 65536, the rest 0.
 *
 *   Sampling.  p = base + disp per axis; x0 = px >> 8, fx = px & 255, likewise y0, fy; with pAB the source byte at
 *   (x0 + A, y0 + B), or `fill` where that lies outside the image,
 *       v = ((256 - fx)(256 - fy) p00 + fx (256 - fy) p10 + (256 - fx) fy p01 + fx fy p11 + 32768) >> 16.
 *
 * params_dev is int32 [n][12]: {draw id low word, high word, amp_x, amp_y, a0, a1, a2, a3, a4, a5, 0, 0}.
 * field_dev, optional, is int32 [n][2][h][w]: disp (the Q8 displacement before the affine), x plane then y plane.
 *
 * Method (csrc/warp.hip).  One 256-thread workgroup per output image.  The source image is staged in LDS (16-byte loads
 * where its address allows); the first threads draw the control points into LDS, one Philox group each; the horizontal
 * B-spline sums per control row are formed in LDS as int32; each thread then forms four adjacent output pixels and
 * stores one aligned dword.  Two barriers, no atomics, nothing written outside out_dev's n images (and field_dev's).
 *
 * The call is context-free, like siggan_dtw_pairs: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: work is enqueued on `stream` and the host is never synchronised, 0 = OK / negative = SIGGAN_E_* with
 * the message in siggan_last_error(), the caller's current device is restored.  Adding this header did not change
 * SIGGAN_ABI_VERSION: it only adds a symbol.
 */
#ifndef SIGGAN_WARP_H
#define SIGGAN_WARP_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_WARP_MAX_SIZE 128
#define SIGGAN_WARP_PARAMS 12
#define SIGGAN_WARP_STREAM 0x57415250u              /* the stream id of the control-point draws ("WARP") */
#define SIGGAN_WARP_MAX_AMP(cell) ((cell) * 512 / 5) /* floor(0.4 * cell * 256): 819, 1638, 3276 */
#define SIGGAN_WARP_MAX_CTRL 8192                   /* 32 pixels: keeps the horizontal sums inside int32 at cell 32 */

/* src_dev (n_src, h, w) uint8 -> out_dev (n, h, w) uint8, one kernel on `stream`.  index_dev (n) int32, ctrl_dev and
 * field_dev may be null.  SIGGAN_E_INVALID, nothing enqueued: a null src_dev, params_dev or out_dev, n outside 1..2^20,
 * n_src < 1, h outside 1..128, w outside 4..128 or not a multiple of 4, a cell other than 8, 16, 32, fill outside 0..255,
 * src_dev, out_dev or field_dev not 4-byte aligned or ctrl_dev not 2-byte aligned, out_dev's n images overlapping
 * src_dev's n_src. */
int siggan_warp_u8(int32_t device, const uint8_t *src_dev, int64_t n_src, const int32_t *index_dev, const int32_t *params_dev,
                   const int16_t *ctrl_dev, uint8_t *out_dev, int32_t *field_dev, int32_t n, int32_t h, int32_t w, int32_t cell,
                   int32_t fill, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_WARP_H */
