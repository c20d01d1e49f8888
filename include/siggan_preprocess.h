/*
 * siggan_preprocess.h -- C ABI of scan preprocessing on the MI355X: from raw grayscale scans of any size to the 64 x 64 or
 * 128 x 128 byte images every other part of the library reads.  Six stages, each defined by exact integer arithmetic
 * (tests/preprocesscommon.py is the restatement the kernels equal bit for bit):
 *   1. denoise   3 x 3 binomial blur (1 2 1)^2 / 16 with rounding, reflection without the edge; then a grey opening with
 *                the three-pixel element {(y-1, x), (y, x-1), (y, x)}: min, then max, positions outside the image skipped;
 *   2. validate  WHITE = #{pixel > 127} of the denoised scan (the caller decides what to reject);
 *   3. crop      ink is pixel <= 127; 8-connected components of at least min_pixels PIXELS are kept; the crop is their
 *                bounding box widened by `margin`, clamped the way the reference clamps it; none kept: the whole scan;
 *   4. resize    scale = min(T / cw, T / ch), nw = int(cw * scale), nh = int(ch * scale) in IEEE doubles; the exact box
 *                average with one rounding; pasted at ((T - nw) / 2, (T - nh) / 2) on paper (255);
 *   5. centre    integer centroid of 255 - canvas moved to (T / 2, T / 2) by a whole-pixel shift, paper shifted in;
 *   6. equalise  CLAHE on an 8 x 8 grid, clip limit 2.0: clipped histograms, redistribution, bilinear blend of four LUTs.
 * Which of these follow OpenCV's rule and which replace it is tabulated in DESIGN.md; agreement with an OpenCV build is not
 * measured.
 *
 * Method (csrc/preprocess.hip): three kernels.  k_pp_denoise works on 64 x 64 tiles with the three stencils fused in LDS
 * and leaves one WHITE partial per tile; k_pp_label labels horizontal ink runs of one scan per workgroup with a lock-free
 * union-find in the workspace (links point to the smaller run, atomic min), sums areas and takes the box of the kept
 * components; k_pp_finish, one workgroup per scan, does stages 4 to 6 in LDS.  Integers throughout but for the four
 * doubles of stage 4; min, max and integer add do not depend on order, so equal input gives equal output bits.
 *
 * The batch is ragged: `pool` holds the scans back to back, `geom` says where.  The call is context-free, like
 * siggan_components_u8: `device` is the HIP ordinal the pointers belong to.  Conventions are those of siggan.h: it enqueues
 * on `stream` and never synchronises the host, allocates nothing, 0 = OK / negative = SIGGAN_E_* with the message in
 * siggan_last_error(), the caller's current device is restored.  Adding this header did not change SIGGAN_ABI_VERSION: it
 * only adds symbols.
 */
#ifndef SIGGAN_PREPROCESS_H
#define SIGGAN_PREPROCESS_H

#include <stddef.h>

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_PP_MIN_SIDE 16
#define SIGGAN_PP_MAX_SIDE 1024
#define SIGGAN_PP_MAX_MARGIN 64
#define SIGGAN_PP_MAX_BATCH 65536

/* columns of geom */
enum { SIGGAN_PP_GEOM_OFFSET, SIGGAN_PP_GEOM_HEIGHT, SIGGAN_PP_GEOM_WIDTH, SIGGAN_PP_GEOM_MIN_PIXELS, SIGGAN_PP_GEOM_COUNT };

/* bits of stats column SIGGAN_PP_STATUS */
#define SIGGAN_PP_NO_BBOX 1    /* crop asked for, no component of min_pixels pixels: the whole scan was used */
#define SIGGAN_PP_DEGENERATE 2 /* the resized side would be 0 pixels: out (and canvas) are all 255 */
#define SIGGAN_PP_OVERFLOW 4   /* the labelling's safety bound was hit, which no input should do; no other output counts */

/* columns of stats_dev */
enum {
    SIGGAN_PP_STATUS,     /* the bits above */
    SIGGAN_PP_WHITE,      /* pixels > 127 after stage 1 */
    SIGGAN_PP_COMPONENTS, /* 8-connected ink components after stage 1 (0 with crop off: nothing is labelled) */
    SIGGAN_PP_KEPT,       /* those of at least min_pixels pixels */
    SIGGAN_PP_CROP_X,     /* the crop */
    SIGGAN_PP_CROP_Y,
    SIGGAN_PP_CROP_W,
    SIGGAN_PP_CROP_H,
    SIGGAN_PP_NEW_W,      /* the resized crop (0, 0 when DEGENERATE) */
    SIGGAN_PP_NEW_H,
    SIGGAN_PP_SHIFT_X,    /* stage 5's shift (0, 0 with center off, without ink or when DEGENERATE) */
    SIGGAN_PP_SHIFT_Y,
    SIGGAN_PP_M00,        /* sum of 255 - canvas before the shift (0 with center off or when DEGENERATE) */
    SIGGAN_PP_COUNT
};

typedef struct siggan_preprocess_options {
    int32_t target;   /* 64 or 128 */
    int32_t denoise;  /* stage 1 on (non-zero) / off */
    int32_t crop;     /* stage 3 */
    int32_t center;   /* stage 5 */
    int32_t equalize; /* stage 6 */
    int32_t margin;   /* stage 3's margin, 0 .. SIGGAN_PP_MAX_MARGIN; the reference uses 5 */
} siggan_preprocess_options;

/* Bytes of workspace for n scans in a pool of total_pixels bytes: the denoised pool, row masks, run labels and areas, the
 * per-tile WHITE partials and the per-scan boxes.  0 when n is outside 1..SIGGAN_PP_MAX_BATCH or total_pixels < 1. */
size_t siggan_preprocess_workspace(int64_t total_pixels, int32_t n);

/* pool_dev       uint8, total_pixels bytes: scan i is rows of geom[i].width bytes from byte geom[i].offset on.
 * geom_host      (n, 4) int64 {offset, height, width, min_pixels} in host memory: read during the call for validation and
 *                grid sizing, not kept;
 * geom_dev       the same table in device memory, which the kernels read.
 * out_dev        (n, T, T) uint8.   stats_dev (n, SIGGAN_PP_COUNT) int32.
 * denoised_dev   optional, total_pixels bytes: stage 1's result, laid out like the pool (bytes between scans untouched).
 * canvas_dev     optional, (n, T, T) uint8: the image before stage 6.
 * workspace_dev  at least siggan_preprocess_workspace(total_pixels, n) bytes, 8-byte aligned; its content on entry does
 *                not matter.
 * SIGGAN_E_INVALID, nothing enqueued: n outside 1..SIGGAN_PP_MAX_BATCH, a null pointer among pool, geom_host, geom_dev,
 * options, out_dev (missing out_dev), stats_dev (missing stats_dev) and workspace_dev, target not 64 or 128, margin outside
 * 0..64, a height or width outside 16..1024, min_pixels < 1, offsets that are negative, not ascending, overlap or run past
 * total_pixels, a workspace that is too small or not 8-byte aligned, stats_dev not 4-byte aligned. */
int siggan_preprocess_u8(int32_t device, const uint8_t *pool_dev, int64_t total_pixels, const int64_t *geom_host,
                         const int64_t *geom_dev, int32_t n, const siggan_preprocess_options *options, uint8_t *out_dev,
                         int32_t *stats_dev, uint8_t *denoised_dev, uint8_t *canvas_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_PREPROCESS_H */
