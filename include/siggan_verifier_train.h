/*
 * siggan_verifier_train.h -- C ABI of the Siamese signature verifier's TRAIN step on the MI355X: train-mode forward, BCE (+
 * contrastive) loss, backward and Adam, as the reference's train_epoch does per batch (signature_verifier_train.py:376-449).
 *
 * The network is the one of siggan_verifier.h.  In train mode
 *   - the encoder runs on x1, then on x2: BatchNorm batch statistics are taken PER HALF over that half's n_pairs images
 *     (biased variance for the normalisation, unbiased for the running tensors, momentum 0.1), and the running tensors are
 *     updated twice per step, from x1 and then from x2;
 *   - Dropout(0.5) follows fc1 + ReLU (separately per half), Dropout(0.3) sits in the classifier; multiplier keep / (1 - p);
 *   - loss = BCELoss(similarity, y) [+ 0.5 * mean(y D^2 + (1 - y) clamp(2 - D, 0)^2), D = ||e1 - e2 + 1e-6||_2].
 * One deliberate deviation: the three conv biases sit in front of a train-mode BatchNorm, their gradient is mathematically
 * zero and the library writes exactly 0 for it, so those biases and their Adam moments never move.
 * Equal maxima of a pooling window route the gradient to the first element in (dy, dx) order (torch's rule).
 *
 * fp32 only.  Every reduction (BatchNorm sums, split-K, weight gradients, batch sums) has a fixed order -- partial slabs and
 * an ordered sum, no float atomics -- so equal inputs, masks and state give equal bits.
 *
 * Conventions are those of siggan_verifier.h: plain pointers, everything enqueued on `stream`, no host synchronisation,
 * 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the caller's device restored.  The header only adds
 * symbols: SIGGAN_ABI_VERSION is unchanged.
 */
#ifndef SIGGAN_VERIFIER_TRAIN_H
#define SIGGAN_VERIFIER_TRAIN_H

#include "siggan_verifier.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_VT_PARAM_TENSORS 20   /* SiameseNetwork.named_parameters() */
#define SIGGAN_VT_METRICS 4          /* loss, bce, contrastive, n_correct */

typedef struct siggan_verifier_trainer siggan_verifier_trainer;

/* Caller-owned device memory (as siggan_storage is for the GAN).  The four arenas are flat fp32 and hold the 20 parameter
 * tensors back to back in named_parameters() order (siggan_verifier_trainer_param_span gives every tensor's place):
 *   encoder.conv1.weight, .bias, encoder.bn1.weight, .bias, conv2 / bn2, conv3 / bn3 likewise, encoder.fc1.weight, .bias,
 *   encoder.fc2.weight, .bias, classifier.0.weight, .bias, classifier.3.weight, .bias
 * num_batches_tracked is host state: every step adds 2 to it. */
typedef struct siggan_verifier_train_storage {
    float *params, *grads, *exp_avg, *exp_avg_sq;
    float *bn1_running_mean, *bn1_running_var, *bn2_running_mean, *bn2_running_var, *bn3_running_mean, *bn3_running_var;
    float bn_eps;                    /* 1e-5 */
} siggan_verifier_train_storage;

/* max_pairs in 1..1024.  All workspace (about 4.7 MB per pair + 76 KB of weight packs + the weight-gradient slabs, 0.6 MB per
 * pair) is allocated here, once. */
int siggan_verifier_trainer_create(int32_t device, int32_t embedding_dim, int32_t max_pairs, siggan_verifier_trainer **out);
int siggan_verifier_trainer_destroy(siggan_verifier_trainer *t);
int64_t siggan_verifier_trainer_param_count(const siggan_verifier_trainer *t);
/* first element and element count of parameter tensor `index` (0..19) inside the arenas */
int siggan_verifier_trainer_param_span(const siggan_verifier_trainer *t, int32_t index, int64_t *offset, int64_t *count);
/* keeps the pointers; resets the Adam step count to `adam_step` steps already taken (0 for fresh moments) */
int siggan_verifier_trainer_bind(siggan_verifier_trainer *t, const siggan_verifier_train_storage *storage, int64_t adam_step);
/* the counter-based RNG (rng.h) of the dropout keep masks that are not handed in: mask element i of a site at step k is
 * Philox(seed; counter = (i / 4, site stream, offset + k)).  The three sites (fc dropout of x1, of x2, classifier) have
 * distinct streams; every _grads call advances k. */
int siggan_verifier_trainer_seed(siggan_verifier_trainer *t, uint64_t seed, uint64_t offset);

/* Train-mode forward, losses and backward; writes the whole gradient arena (nothing is accumulated) and updates the six
 * running tensors.  x1 / x2: n_pairs images each in `fmt`; labels (n_pairs) fp32 1 / 0.
 * fc_keep_masks (2 * n_pairs, 512), x1's rows first, and cls_keep_masks (n_pairs, 64): fp32 1 / 0 keep masks, or NULL to
 * draw them.  metrics_dev (4 floats, may be NULL): loss, bce, contrastive (0 without use_contrastive), n_correct =
 * #{(similarity > 0.5) == y}. */
int siggan_verifier_train_grads(siggan_verifier_trainer *t, const void *x1_dev, const void *x2_dev, int32_t fmt,
                                const float *labels_dev, int32_t n_pairs, const float *fc_keep_masks,
                                const float *cls_keep_masks, int32_t use_contrastive, float *metrics_dev, void *stream);
/* One torch.optim.Adam update over the arena from the gradient arena (no weight decay, no amsgrad); the step count lives on
 * the host and the bias corrections are formed there in double, as the GAN's fused update does. */
int siggan_verifier_train_apply(siggan_verifier_trainer *t, double lr, double beta1, double beta2, double eps, void *stream);
/* _grads followed by _apply */
int siggan_verifier_train_step(siggan_verifier_trainer *t, const void *x1_dev, const void *x2_dev, int32_t fmt,
                               const float *labels_dev, int32_t n_pairs, const float *fc_keep_masks,
                               const float *cls_keep_masks, int32_t use_contrastive, double lr, double beta1, double beta2,
                               double eps, float *metrics_dev, void *stream);
/* test hook: stage `name` of the last _grads call; n is the stage's element count.
 *   "route1" (2B,32,32,32) / "route2" (2B,64,16,16) / "route3" (2B,128,8,8): uint8 per pooled element in NCHW order, 0..3 =
 *       the winning element of the 2x2 window in (dy, dx) row-major order, 4 = the window's max is not positive
 *   "fc1_mask" (2B,512), "cls_mask" (B,64): uint8 ReLU decisions;  "fc_keep" (2B,512), "cls_keep" (B,64): uint8 keep masks used
 *   "e1", "e2" (B,E), "similarity" (B), "distance" (B): fp32 */
int siggan_verifier_train_debug(siggan_verifier_trainer *t, const char *name, void *out_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_TRAIN_H */
