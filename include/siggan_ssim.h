/*
 * siggan_ssim.h -- C ABI of the structural similarity index (SSIM, Wang et al. 2004) between byte images on the MI355X:
 * the one measure of the evaluation that compares two images pixel by pixel and needs no network weights.  Every pair of
 * two sets is scored on the device, so the bytes of siggan_g_generate_u8 and the decoded real cache never leave it; only a
 * matrix, or one best value and index per row, reaches the host.
 *
 * Definition.  Single scale, L = 255, two uint8 images of equal size (h, w).  All five local moments use one window g (x) g:
 * g is 11 taps of exp(-(k - 5)^2 / (2 * 1.5^2)), normalised by their sum in double on the host and rounded to float once
 * (siggan_ssim_window).  The window is applied at "valid" positions only: (h - 10) x (w - 10) maps, no padding.  With x, y
 * the bytes as float:
 *     mu_x = G * x, mu_y = G * y
 *     var_x = G * (x x) - mu_x mu_x, var_y likewise, cov = G * (x y) - mu_x mu_y
 *     C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2
 *     s = ((2 (mu_x mu_y) + C1) (2 cov + C2)) / ((mu_x mu_x + mu_y mu_y + C1) (var_x + var_y + C2))
 *     SSIM = sum(s) / (float)((h - 10)(w - 10))
 * in fp32, one IEEE division per map element and one by the count.
 *
 * Method (csrc/ssim.hip).  mu and var depend on one image, so they are PREPARED once per image (siggan_ssim_prepare_u8) and
 * a set is prepared once however many sets it is later compared with.  Per pair only G * (x y) is formed.  One device
 * function filters a stream of rows -- fmaf chains with the taps ascending, horizontal then vertical -- for x and x x in the
 * prepare kernel and for x y in the pair kernel; the library is built with -ffp-contract=off, so equal expressions give
 * equal bits: SSIM(x, x) is exactly 1.0f, SSIM(x, y) and SSIM(y, x) are the same bits, and a pair's value does not depend on
 * where it stands in a batch, on the mode or on how the columns were split over workgroups.  No float atomics, no global
 * atomics: equal input gives equal output bits whatever the scheduling.
 *
 * The calls are context-free, like siggan_components_u8: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: work is enqueued on `stream` and the host is never synchronised, 0 = OK / negative = SIGGAN_E_* with
 * the message in siggan_last_error(), the caller's current device is restored.  Adding this header did not change
 * SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_SSIM_H
#define SIGGAN_SSIM_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_SSIM_TAPS 11
#define SIGGAN_SSIM_SIGMA 1.5
#define SIGGAN_SSIM_MIN_HEIGHT 11 /* one row of windows */
#define SIGGAN_SSIM_MIN_WIDTH 12  /* the smallest multiple of 4 that holds a window */
#define SIGGAN_SSIM_MAX_SIZE 128

enum {
    SIGGAN_SSIM_ALL,      /* every a_i against every b_j */
    SIGGAN_SSIM_SAME_SET, /* b is a: best skips j = i */
    SIGGAN_SSIM_PAIRED    /* a_i against b_i only */
};

/* The 11 taps as the kernels use them.  Needs no device. */
int siggan_ssim_window(float w[SIGGAN_SSIM_TAPS]);

/* Bytes of the maps of n images of (h, w): n * 2 * (h - 10) * (w - 10) * 4.  SIGGAN_E_INVALID (negative) for n < 1 or a size
 * siggan_ssim_prepare_u8 refuses. */
int64_t siggan_ssim_maps_bytes(int32_t n, int32_t h, int32_t w);

/* u8_dev (n, h, w) uint8 -> maps_dev (n, 2, h - 10, w - 10) fp32: plane 0 mu, plane 1 var.  One kernel on `stream`.
 * SIGGAN_E_INVALID, nothing enqueued: n < 1, h outside 11..128, w outside 12..128 or not a multiple of 4, a null pointer, a
 * pointer that is not 4-byte aligned. */
int siggan_ssim_prepare_u8(int32_t device, const uint8_t *u8_dev, int32_t n, int32_t h, int32_t w, float *maps_dev, void *stream);

/* a_u8 (na, h, w) with a_maps, b_u8 (nb, h, w) with b_maps, both prepared by siggan_ssim_prepare_u8.  Outputs, each optional
 * but at least one given:
 *   SIGGAN_SSIM_ALL       matrix (na, nb) fp32; best (na) fp32 / best_index (na) int32: each row's highest SSIM and its column,
 *                         equal values resolved to the lower column.
 *   SIGGAN_SSIM_SAME_SET  b is a: b_u8 / b_maps are null or a's, nb == na.  The matrix is complete (its diagonal is 1.0);
 *                         best skips j = i, so na = 1 gives -1.0 / -1.
 *   SIGGAN_SSIM_PAIRED    nb == na; matrix is (na), entry i = SSIM(a_i, b_i); best / best_index are refused.
 * With only best / best_index asked for no matrix is formed anywhere: every workgroup keeps one key per row and slice of
 * columns in a workspace the call takes from and returns to the stream's memory pool.
 * SIGGAN_E_INVALID, nothing enqueued and nothing allocated: na or nb < 1, a size siggan_ssim_prepare_u8 refuses, a mode outside
 * the enum, no output, a missing input, a pointer that is not 4-byte aligned, nb != na or a foreign b where the mode
 * forbids it, best pointers in SIGGAN_SSIM_PAIRED. */
int siggan_ssim_pairs(int32_t device, const uint8_t *a_u8, const float *a_maps, int32_t na, const uint8_t *b_u8,
                      const float *b_maps, int32_t nb, int32_t h, int32_t w, int32_t mode, float *matrix, float *best,
                      int32_t *best_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_SSIM_H */
