/*
 * siggan_dtw.h -- C ABI of elastic signature matching on the MI355X: banded dynamic time warping (DTW) between the column
 * profiles of byte images.  A signature is read left to right as a sequence of per-column measurements and two such
 * sequences are aligned elastically, so the same signature written a few pixels to the side, or slightly wider, stays close
 * where a pixelwise measure (siggan_ssim.h) sees another image.  It needs no network weights.  Every pair of two sets is
 * scored on the device; only a matrix, or one best value and index per row, reaches the host.
 *
 * Definition (exact, integers only).  Ink is byte < threshold.  Column x of an image of height h gets four bytes:
 *     c  the number of ink pixels in the column                               (0 .. h)
 *     t  the row of its first ink pixel, h / 2 (integer division) if it has none
 *     b  the row of its last ink pixel,  h / 2 if it has none
 *     r  the number of vertical ink runs in it                                (0 .. ceil(h / 2))
 * packed as one little-endian dword c | t << 8 | b << 16 | r << 24: a profile set is (n, w) uint32, or (n, w, 4) uint8.
 * The local cost between column i of a and column j of b is d(i, j) = |dc| + |dt| + |db| + |dr|, a four-byte sum of
 * absolute differences.  With 0 <= band <= w - 1, over the cells with |i - j| <= band:
 *     D(0, 0) = d(0, 0),     D(i, j) = d(i, j) + min(D(i - 1, j), D(i, j - 1), D(i - 1, j - 1))
 * where cells outside the band or the grid do not exist, and DTW(a, b) = D(w - 1, w - 1) as int32.  It follows that
 * DTW(x, x) = 0, DTW(a, b) = DTW(b, a), band 0 is the plain sum of d(i, i), a larger band never increases the value, and the
 * value is at most 128 * 446 = 57088: it does not fit 16 bits.  Only the writing direction is elastic: a vertical
 * displacement is costed through t and b, on purpose.  The two sets may come from images of different heights.
 *
 * Method (csrc/dtw.hip).  siggan_dtw_profiles_u8: one thread per column walks its rows.  siggan_dtw_pairs: a wave64 is a
 * systolic array.  Lane i keeps column i of a in a register; b's columns enter at lane 0, one per step, and travel one lane
 * per step (a DPP wave shift); a lane keeps D(i, j - 1) from its own previous step, takes D(i - 1, j) from the lane below
 * it by the same shift, and remembers last step's value of that as D(i - 1, j - 1).  No LDS, no barrier.  Beyond 64 columns
 * the rows are done in two strips of 64: the wave keeps row D(63, .) of the first strip in two registers and feeds it into
 * lane 0 of the second.  A cell outside the band is set to a sentinel that no existing cell ever reads as its minimum, so
 * the result does not depend on its value.  Integers only and no atomics of any kind: equal input gives equal output
 * whatever the scheduling, and a pair's value does not depend on the mode or on its neighbours in the launch.
 *
 * The calls are context-free, like siggan_ssim_pairs: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: work is enqueued on `stream` and the host is never synchronised, 0 = OK / negative = SIGGAN_E_* with
 * the message in siggan_last_error(), the caller's current device is restored.  Adding this header did not change
 * SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_DTW_H
#define SIGGAN_DTW_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_DTW_MAX_SIZE 128

enum {
    SIGGAN_DTW_ALL,      /* every a_i against every b_j */
    SIGGAN_DTW_SAME_SET, /* b is a: best skips j = i */
    SIGGAN_DTW_PAIRED    /* a_i against b_i only */
};

/* u8_dev (n, h, w) uint8 -> profiles_dev (n, w) uint32, the packed column profiles above.  One kernel on `stream`.
 * SIGGAN_E_INVALID, nothing enqueued: a null pointer, n < 1, h outside 1..128, w outside 4..128 or not a multiple of 4,
 * threshold outside 1..255, a pointer that is not 4-byte aligned. */
int siggan_dtw_profiles_u8(int32_t device, const uint8_t *u8_dev, int32_t n, int32_t h, int32_t w, int32_t threshold,
                           uint32_t *profiles_dev, void *stream);

/* a_prof (na, w), b_prof (nb, w): profiles made by siggan_dtw_profiles_u8.  Outputs, each optional but at least one given:
 *   SIGGAN_DTW_ALL       matrix (na, nb) int32; best (na) int32 / best_index (na) int32: each row's lowest distance and its
 *                        column, equal values resolved to the lower column.
 *   SIGGAN_DTW_SAME_SET  b is a: b_prof is null or a's, nb == na.  The matrix is complete (its diagonal is 0); best skips
 *                        j = i, so na = 1 gives -1 / -1.
 *   SIGGAN_DTW_PAIRED    nb == na; matrix is (na), entry i = DTW(a_i, b_i); best / best_index are refused.
 * With only best / best_index asked for no matrix is formed anywhere: every wave keeps one key per row and slice of columns
 * in a workspace the call takes from and returns to the stream's memory pool, and a second kernel takes the slices in order.
 * SIGGAN_E_INVALID, nothing enqueued and nothing allocated: na or nb < 1, w outside 4..128 or not a multiple of 4, band
 * outside 0..w - 1, a mode outside the enum, no output, a missing input, a pointer that is not 4-byte aligned, nb != na or a
 * foreign b where the mode forbids it, best pointers in SIGGAN_DTW_PAIRED. */
int siggan_dtw_pairs(int32_t device, const uint32_t *a_prof, int32_t na, const uint32_t *b_prof, int32_t nb, int32_t w,
                     int32_t band, int32_t mode, int32_t *matrix, int32_t *best, int32_t *best_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_DTW_H */
