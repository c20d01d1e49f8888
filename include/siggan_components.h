/*
 * siggan_components.h -- C ABI of connected-component labelling of byte images on the MI355X: what a count of ink pixels
 * (siggan_image_stats, siggan_g_generate_u8's counters) cannot say.  Per image it gives the number of ink components, the
 * largest one, how much ink sits in components below a minimum area, the bounding box of the rest, a canonical label map
 * and a cleaned copy ("despeckle").  The bytes of siggan_g_generate_u8 are labelled where they are: only the nine counters
 * per image need to reach the host.
 *
 * Ink is byte < threshold, the rule of siggan_gather_u8's binarize and of siggan_d_score_u8.  A component is a maximal set
 * of ink pixels connected under `connectivity` (8: edges and corners, what OpenCV's contours use for foreground; 4: edges
 * only).  A component is SMALL iff its pixel count is < min_area.
 *
 * Method (csrc/components.hip): one workgroup per image, everything in LDS.  A wave64 ballot turns each row into an ink
 * mask; a RUN is a maximal horizontal stretch of ink, at most width / 2 per row, and the unit that is labelled.  Runs of
 * neighbouring rows that touch are joined by a lock-free union-find whose links always point to the smaller index (LDS
 * atomic min), so the root of a component is its first run in raster order and the label is that run's first pixel.
 * Areas are summed with LDS atomic adds.  Integers only, no global atomics, no floating point: min and add do not depend
 * on order, so equal input gives equal output bits whatever the scheduling.  Nothing iterates to a fixed point; every
 * loop is nevertheless bounded by the number of run slots, and an image whose bound is hit (a bug, not an input) gets
 * COMPONENTS = -1 and no other output.
 *
 * The call is context-free, like siggan_select_topk: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: it enqueues one kernel on `stream` and never synchronises the host, 0 = OK / negative = SIGGAN_E_*
 * with the message in siggan_last_error(), the caller's current device is restored.  Adding this header did not change
 * SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_COMPONENTS_H
#define SIGGAN_COMPONENTS_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_CC_MAX_SIZE 128

/* columns of stats_dev */
enum {
    SIGGAN_CC_INK,              /* ink pixels */
    SIGGAN_CC_COMPONENTS,       /* components (-1: the kernel's safety bound was hit, which no input should do) */
    SIGGAN_CC_LARGEST,          /* pixel count of the largest component, 0 without ink */
    SIGGAN_CC_SMALL_COMPONENTS, /* components with fewer than min_area pixels */
    SIGGAN_CC_SMALL_INK,        /* the pixels in them */
    SIGGAN_CC_X0,               /* inclusive bounding box of all pixels of components that are not small; */
    SIGGAN_CC_Y0,               /* all four are -1 when there is none */
    SIGGAN_CC_X1,
    SIGGAN_CC_Y1,
    SIGGAN_CC_COUNT
};

/* u8_dev (batch, height, width) uint8.  Outputs, each optional but at least one given:
 *   stats_dev (batch, SIGGAN_CC_COUNT) int32: the counters above;
 *   root_dev  (batch, height, width) int32: -1 for background, else the smallest linear index y * width + x of the pixel's
 *             component -- a label that depends on nothing but the image;
 *   clean_dev (batch, height, width) uint8: the input byte, except that every pixel of a small component becomes `fill`;
 *             grey levels of kept components are untouched.  clean_dev == u8_dev (in place) is allowed, any other overlap
 *             of buffers is the caller's error.
 * SIGGAN_E_INVALID, nothing enqueued: batch < 1, height outside 1..128, width outside 4..128 or not a multiple of 4,
 * threshold outside 1..255, connectivity not 4 or 8, min_area < 1, fill outside threshold..255 (a cleaned pixel must not
 * be ink), no output pointer, a pointer that is not 4-byte aligned. */
int siggan_components_u8(int32_t device, const uint8_t *u8_dev, int32_t batch, int32_t height, int32_t width,
                         int32_t threshold, int32_t connectivity, int32_t min_area, int32_t fill,
                         int32_t *stats_dev, int32_t *root_dev, uint8_t *clean_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_COMPONENTS_H */
