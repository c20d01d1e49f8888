/*
 * siggan_resize.h -- C ABI of Pillow's antialiased bilinear resize for single-channel images on the MI355X: the step
 * torchvision's transforms.Resize((64, 64)) takes on a PIL image before the Siamese verifier sees it.  With it the 128x128
 * Generator's bytes (siggan_g_generate_u8) reach siggan_verifier_embed without leaving the device.
 *
 * The map is Image.resize(size, Image.BILINEAR) for mode 'L' (ImagingResample, Resample.c): a triangle filter whose support
 * widens with the downscale factor, applied as two separable passes, the horizontal one first.  Per axis and output index xx:
 *     scale = in / out, filterscale = max(scale, 1), support = filterscale, ksize = 2 * ceil(support) + 1
 *     center = (xx + 0.5) * scale
 *     xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in) - xmin       (the window)
 *     w[x] = triangle((x + xmin - center + 0.5) * (1 / filterscale)), x in [0, xmax), divided by their sum    (double)
 *     kk[x] = (int)(0.5 + w[x] * 2^22)            (the 8-bit path's fixed point; -0.5 for a negative weight, which a
 *                                                  triangle never gives)
 * The byte path accumulates in int32 from 1 << 21, shifts right by 22, clips to 0 .. 255 and stores the horizontal pass as
 * BYTES before the vertical pass reads them -- that rounding is part of the result.  A pass whose axis does not change is
 * skipped.  The fp32 paths apply the same linear map y = R_h x R_w^T with the un-quantised weights rounded to fp32, an fp32
 * intermediate and ascending tap order, and its exact transpose dx = R_h^T dy R_w as a gather in ascending output order.
 *
 * Conventions are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises the
 * host, 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's current device is restored.
 * A context caches one coefficient table per (in, out) axis pair: the FIRST call that needs a new pair builds it on the
 * host, allocates it on the device and uploads it with a blocking copy (so that call must not run inside a stream
 * capture); every later call only launches.  A context serves one host thread at a time.  No atomics, a fixed order of
 * every sum: equal input gives bit-equal output.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_RESIZE_H
#define SIGGAN_RESIZE_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_RESIZE_MAX_IN  1024
#define SIGGAN_RESIZE_MAX_OUT 128

typedef struct siggan_resize siggan_resize;

int siggan_resize_create(int32_t device, siggan_resize **out);
int siggan_resize_destroy(siggan_resize *ctx);

/* Host only, needs no GPU.  ksize of the axis pair (in, out), or SIGGAN_E_INVALID unless 1 <= in <= SIGGAN_RESIZE_MAX_IN
 * and 1 <= out <= SIGGAN_RESIZE_MAX_OUT. */
int32_t siggan_resize_ksize(int32_t in, int32_t out);

/* Host only, needs no GPU: the table of the axis pair (in, out) into caller-owned HOST buffers, any of which may be NULL.
 * bounds_out (out, 2) int32: xmin and the window length xmax; kk_out (out, ksize) int32: the 22-bit weights, 0 past the
 * window; kf_out (out, ksize) fp32: the double weights rounded to fp32, 0 past the window.  Sizes as siggan_resize_ksize. */
int siggan_resize_table(int32_t in, int32_t out, int32_t *bounds_out, int32_t *kk_out, float *kf_out);

/* dst (n, h_out, w_out) uint8 = Pillow's resize of src (n, h_in, w_in) uint8, byte for byte.  n >= 1,
 * 1 <= h_in, w_in <= SIGGAN_RESIZE_MAX_IN, 1 <= h_out, w_out <= SIGGAN_RESIZE_MAX_OUT, else SIGGAN_E_INVALID.  src and dst
 * must not overlap. */
int siggan_resize_u8(siggan_resize *ctx, const uint8_t *src_dev, int32_t n, int32_t h_in, int32_t w_in, uint8_t *dst_dev,
                     int32_t h_out, int32_t w_out, void *stream);

/* The same linear map on fp32 images without the byte roundings: dst (n, h_out, w_out) = R_h src R_w^T.  Sizes as above. */
int siggan_resize_f32(siggan_resize *ctx, const float *src_dev, int32_t n, int32_t h_in, int32_t w_in, float *dst_dev,
                      int32_t h_out, int32_t w_out, void *stream);

/* Its exact transpose: dx (n, h_in, w_in) = R_h^T dy R_w for dy (n, h_out, w_out), the gradient of a scalar with respect to
 * siggan_resize_f32's input given the one with respect to its output.  Every element of dx is written.  Sizes as above. */
int siggan_resize_f32_adjoint(siggan_resize *ctx, const float *dy_dev, int32_t n, int32_t h_out, int32_t w_out, float *dx_dev,
                              int32_t h_in, int32_t w_in, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_RESIZE_H */
