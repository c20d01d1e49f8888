/*
 * siggan_strokes.h -- C ABI of stroke geometry of byte images on the MI355X: what a count of ink pixels and a count of ink
 * components (siggan_components.h) cannot say -- how thick a stroke is.  Per image it gives the exact squared Euclidean
 * distance map of the ink, the skeleton (centre line) by Guo-Hall parallel thinning, counters of both (skeleton length, line
 * ends, junction pixels, a histogram of local pen widths) and a redraw of the skeleton at a chosen pen width.  The bytes of
 * siggan_g_generate_u8 are measured where they are: only the 23 counters per image need to reach the host.
 *
 * Ink is byte < threshold, the rule of siggan_gather_u8's binarize, siggan_d_score_u8 and siggan_components_u8.  Pixels
 * outside the image are background ("the paper goes on"), for the distance map and for the thinning alike, so every
 * quantity is defined for every input, an all-ink image included.
 *
 * Distance map.  D2(p) is the squared Euclidean distance from ink pixel p to the nearest background pixel, 0 on background,
 * at most 64 * 64 = 4096.  Exact in integers: g(x, y), the distance to the nearest background pixel of the column, then the
 * minimum over x' of (x - x')^2 + g(x', y)^2 along the row.
 *
 * Skeleton.  Guo & Hall, "Parallel thinning with two-subiteration algorithms" (CACM 1989), algorithm A1.  The neighbours of P
 * are named clockwise from north: P2 N, P3 NE, P4 E, P5 SE, P6 S, P7 SW, P8 W, P9 NW (north is the row above).
 *   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
 *   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
 * A pass is two sub-iterations.  The first deletes every ink pixel with C == 1, 2 <= N <= 3 and ((P2|P3|!P5) & P4) == 0, the
 * second every one with C == 1, 2 <= N <= 3 and ((P6|P7|!P9) & P8) == 0; each reads the state the previous one left and
 * deletes all its pixels at once.  Passes repeat until one whole pass deletes nothing; that pass is counted.  The result
 * depends on nothing but the image.
 *
 * Pen width.  A skeleton pixel with (k - 1)^2 < D2 <= k^2 stands for a local pen width of 2k - 1.  An axis-aligned bar of
 * width W lands in bin ceil(W / 2), so EVEN WIDTHS READ ONE PIXEL LOW (a bar of width 4 reads 3): a centre line of an even
 * stroke lies half a pixel off the middle.  This is documented, not corrected.
 *
 * Method (csrc/strokes.hip): one workgroup per image, everything in LDS, integers only, no floating point, no global atomics.
 * A wave64 ballot turns each row into an ink mask of two 64-bit words; thinning works on whole words (shifts with carry
 * give the eight neighbour planes, a few bitwise adders the conditions), one thread deciding 64 pixels per step.  LDS
 * integer add and max do not depend on order, so equal input gives equal output bits whatever the scheduling.
 *
 * The call is context-free, like siggan_components_u8: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: it enqueues one kernel on `stream` and never synchronises the host, 0 = OK / negative = SIGGAN_E_*
 * with the message in siggan_last_error(), the caller's current device is restored.  Adding this header did not change
 * SIGGAN_ABI_VERSION: it only adds a symbol.
 */
#ifndef SIGGAN_STROKES_H
#define SIGGAN_STROKES_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_SK_MAX_SIZE 128
#define SIGGAN_SK_WIDTH_BINS 16
#define SIGGAN_SK_MAX_RADIUS2 36

/* columns of stats_dev */
enum {
    SIGGAN_SK_INK,             /* ink pixels */
    SIGGAN_SK_SKELETON,        /* skeleton pixels */
    SIGGAN_SK_ENDPOINTS,       /* skeleton pixels with exactly one 8-neighbour on the skeleton */
    SIGGAN_SK_JUNCTION_PIXELS, /* skeleton pixels with three or more 0 -> 1 transitions around the ring P2, P3, ..., P9, P2 taken
                                  on the skeleton: pixels, not crossings -- a crossing may contribute several */
    SIGGAN_SK_PASSES,          /* thinning passes, the last (which deleted nothing) included; -1: the kernel's safety bound of
                                  max(height, width) + 2 passes was reached, which no input should do -- the image then gets no
                                  other output and its other counters are 0 */
    SIGGAN_SK_D2_MAX,          /* the largest D2 over ink pixels, 0 without ink */
    SIGGAN_SK_D2_SKEL_SUM,     /* the sum of D2 over skeleton pixels */
    SIGGAN_SK_WIDTH_HIST,      /* [k - 1], k = 1..16: skeleton pixels with (k - 1)^2 < D2 <= k^2; the last bin also takes */
    SIGGAN_SK_COUNT = SIGGAN_SK_WIDTH_HIST + SIGGAN_SK_WIDTH_BINS /* everything above 15^2.  Integer comparisons, no root */
};

/* u8_dev (batch, height, width) uint8.  Outputs, each optional but at least one given:
 *   stats_dev  (batch, SIGGAN_SK_COUNT) int32: the counters above;
 *   d2_dev     (batch, height, width) int16: the distance map D2;
 *   skel_dev   (batch, height, width) uint8: 1 on the skeleton, 0 elsewhere;
 *   redraw_dev (batch, height, width) uint8: `ink` wherever a skeleton pixel lies within squared distance radius2, `fill`
 *              elsewhere -- a disc dilation of the skeleton clipped to the image; radius2 = 0 gives the skeleton itself.
 *              redraw_dev == u8_dev (in place) is allowed, any other overlap of buffers is the caller's error.
 * SIGGAN_E_INVALID, nothing enqueued: batch < 1, height outside 1..128, width outside 4..128 or not a multiple of 4,
 * threshold outside 1..255, radius2 outside 0..36, ink outside 0..threshold-1, fill outside threshold..255, no output
 * pointer, a pointer that is not 4-byte aligned (2-byte for d2_dev). */
int siggan_strokes_u8(int32_t device, const uint8_t *u8_dev, int32_t batch, int32_t height, int32_t width,
                      int32_t threshold, int32_t radius2, int32_t ink, int32_t fill,
                      int32_t *stats_dev, int16_t *d2_dev, uint8_t *skel_dev, uint8_t *redraw_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_STROKES_H */
