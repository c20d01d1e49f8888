/*
 * siggan_select.h -- C ABI of ranking and gathering on the MI355X: the last two steps of realism-filtered generation
 * (the reference app's "Filter by Realism", app_vanilla_gan_signatures.py:1306-1324: sort the oversampled images by the
 * Discriminator's score, keep the best n).  With siggan_g_generate_u8 and siggan_d_score_u8 (siggan.h) in front of them,
 * the pool of images and its scores never leave the device; only the n selected images and their scores do.
 *
 * Both calls are context-free, like siggan_image_stats: `device` is the HIP ordinal the pointers belong to.  Conventions
 * are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises the host,
 * 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's current device is restored.
 * Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_SELECT_H
#define SIGGAN_SELECT_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_SELECT_MAX 65536

/* index_dev[r], r in [0, k): the index of the score of rank r among scores_dev[0, m), highest first; equal scores keep
 * ascending index order (Python's stable list.sort(key=score, reverse=True)); -0.0 and 0.0 are equal; subnormal scores are
 * ordered by value (the comparison is on the bit patterns, so no flush-to-zero mode has a say).  NaN is not part of the
 * contract.  Rank by counting -- rank(i) = #{j : s_j > s_i or (s_j == s_i and j < i)}, m * m comparisons, the scores
 * tiled through LDS -- and the owner of a rank < k writes index_dev[rank] = i: no atomics, equal input gives equal
 * output.  1 <= k <= m <= SIGGAN_SELECT_MAX, else SIGGAN_E_INVALID. */
int siggan_select_topk(int32_t device, const float *scores_dev, int32_t m, int32_t k, int32_t *index_dev, void *stream);

/* out_dev (k, pixels) uint8: out[r] = pool[index[r]] from pool_dev (m, pixels) uint8, i.e. the selected images in rank
 * order; binarize -1: copied as they are, 0..255: every byte b becomes b < binarize ? 0 : 255 on the way (the rule of
 * siggan_d_score_u8).  Word-wide loads and stores: pixels must be a positive multiple of 4 and both buffers 4-byte
 * aligned; m >= 1, k >= 1, binarize in -1..255, else SIGGAN_E_INVALID.  A row whose index lies outside [0, m) is left
 * unwritten. */
int siggan_gather_u8(int32_t device, const uint8_t *pool_dev, int32_t m, int64_t pixels, const int32_t *index_dev,
                     int32_t k, int32_t binarize, uint8_t *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_SELECT_H */
