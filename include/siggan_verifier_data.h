/*
 * siggan_verifier_data.h -- C ABI of the Siamese verifier trainer's input pipeline on the MI355X: one launch turns a batch
 * of indices into an HBM-resident uint8 image cache into the augmented uint8 images the train step consumes
 * (siggan_verifier_train.h, SIGGAN_VFMT_U8: normalised on load, so the bytes stay bytes from the cache to conv1).
 *
 * What it replaces is the reference's train transform per image (signature_verifier_train.py:541-548) after the decode:
 *   RandomAffine(degrees=5, translate=(0.1, 0.1), scale=(0.9, 1.1)) -> RandomHorizontalFlip(p=0.1)
 * torchvision applies the whole RandomAffine as ONE Pillow Image.transform(AFFINE, NEAREST) with fill 0, then the flip: one
 * resampling stage (the GAN's siggan_augment_batch has two).  The host (signature-gan_amd/verifier_data.py) draws the
 * parameters with the reference DataLoader's RNG protocol and tabulates Pillow's arithmetic; the kernel applies it.
 *
 * Conventions are those of siggan.h: plain pointers, the call enqueues on `stream` and never synchronises the host, 0 = OK /
 * negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's current device is restored.  The header only
 * adds a symbol: SIGGAN_ABI_VERSION is unchanged.
 */
#ifndef SIGGAN_VERIFIER_DATA_H
#define SIGGAN_VERIFIER_DATA_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_PAIRS_IMAGE_SIZE 64   /* the verifier's only image size */

/* out[i] = hflip?( affine( cache[index[i]] ) ) as uint8 (n, 64, 64); the caller passes n = 2 * pairs, x1's rows first, so one
 * launch fills both halves of a train-step batch.  Needs no context.
 *   cache_dev  (n_images, 64, 64) uint8, n_images >= 1; 4-byte aligned.
 *   index_dev  [n] int32; an index outside 0..n_images-1 is clamped to that range (the cache is never read outside).
 *   params_dev [n][8] int32 {mode, a0, a1, a2, a3, a4, a5, flags}, or NULL: plain gather, out[i] = cache[index[i]].
 *       mode 0  copy
 *       mode 1  Pillow's 16.16 fixed-point affine: output (x, y) reads input
 *               ((a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16) when that lies inside the image, else `fill`
 *               (32-bit wrapping arithmetic, arithmetic shift)
 *       mode 2  per-axis source tables: input (tables[i][0][x], tables[i][1][y]); a value outside 0..63 (the host writes
 *               -1) means outside -> `fill`.  Pillow takes this path (ImagingScaleAffine) when the matrix has
 *               m[1] == 0 and m[3] == 0.  With tables_dev == NULL a mode-2 image is all `fill`.
 *       flags bit 0: horizontal flip; it replaces the output column x by 63 - x BEFORE the lookup above, which equals
 *               flipping the transformed image.  Other bits are ignored.
 *   tables_dev [n][2][64] int16 (row 0: source column per output column, row 1: source row per output row), or NULL.
 *   out_dev    (n, 64, 64) uint8, 4-byte aligned: image i starts 4096 * i bytes in; nothing outside those n images is
 *              written.  One thread forms four adjacent pixels and stores them as one aligned 32-bit word.
 *   size       must be SIGGAN_PAIRS_IMAGE_SIZE;  n in 1..2^20;  fill in 0..255 (the reference's RandomAffine leaves fill at
 *              0: corners turn black).
 * Anything else returns SIGGAN_E_INVALID and launches nothing. */
int siggan_pairs_augment(int32_t device, const uint8_t *cache_dev, int64_t n_images, const int32_t *index_dev,
                         const int32_t *params_dev, const int16_t *tables_dev, uint8_t *out_dev, int32_t n, int32_t size,
                         int32_t fill, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_DATA_H */
