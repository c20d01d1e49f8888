/*
 * siggan_verifier.h -- C ABI of the Siamese signature verifier's eval-mode forward on the MI355X.
 *
 * The model is the reference's SiameseNetwork / CNNEncoder (signature_verifier_eval.py:39-179) in eval mode:
 *
 *   encoder  (N,1,64,64) in [-1,1]
 *            Conv2d(1,32,k5,p2)  -> BatchNorm2d (running statistics) -> ReLU -> MaxPool2d(2)      "pool1" (N,32,32,32)
 *            Conv2d(32,64,k5,p2) -> BatchNorm2d -> ReLU -> MaxPool2d(2)                           "pool2" (N,64,16,16)
 *            Conv2d(64,128,k3,p1)-> BatchNorm2d -> ReLU -> MaxPool2d(2)                           "pool3" (N,128,8,8)
 *            flatten (C,H,W) -> Linear(8192,512) + ReLU                                           "fc1"   (N,512)
 *            -> Linear(512,E) -> x / max(||x||_2, 1e-12)
 *   head     |e1 - e2| -> Linear(E,64) + ReLU -> Linear(64,1) -> sigmoid
 *
 * Dropout is the identity in eval mode.  The train step (train-mode forward, BCE + contrastive loss, backward, Adam) is
 * siggan_verifier_train.h's interface; the trainer's input pipeline with the reference's random augmentations is
 * siggan_verifier_data.h's; 16-bit storage is not built.  fp32 only; conv2 / conv3 / fc1 run on v_mfma_f32_32x32x2_f32.
 *
 * Conventions are those of siggan.h: plain pointers and sizes, every call enqueues on `stream` and never synchronises
 * the host, 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), entry points run on the context's
 * device and restore the caller's current device.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds
 * symbols.
 */
#ifndef SIGGAN_VERIFIER_H
#define SIGGAN_VERIFIER_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_E_ARG SIGGAN_E_INVALID   /* every argument error of this header, a call before bind included */

#define SIGGAN_VFMT_F32 0   /* x: fp32 (N,1,64,64), already normalised to [-1,1] */
#define SIGGAN_VFMT_U8  1   /* x: uint8 (N,64,64) as siggan_g_generate_u8 writes it; normalised on load with the
                             * reference's two fp32 operations: v = b / 255.0f; x = (v - 0.5f) / 0.5f */
#define SIGGAN_VERIFIER_MAX_EMBEDDING 8192

typedef struct siggan_verifier siggan_verifier;

/* Device pointers to fp32 tensors in torch's layouts, in state_dict() order.  bind copies / packs everything it needs, so
 * the pointers are not kept. */
typedef struct siggan_verifier_weights {
    const float *conv1_weight, *conv1_bias;                                   /* (32,1,5,5), (32)   */
    const float *bn1_weight, *bn1_bias, *bn1_running_mean, *bn1_running_var;  /* (32) each          */
    const float *conv2_weight, *conv2_bias;                                   /* (64,32,5,5), (64)  */
    const float *bn2_weight, *bn2_bias, *bn2_running_mean, *bn2_running_var;  /* (64) each          */
    const float *conv3_weight, *conv3_bias;                                   /* (128,64,3,3), (128)*/
    const float *bn3_weight, *bn3_bias, *bn3_running_mean, *bn3_running_var;  /* (128) each         */
    const float *fc1_weight, *fc1_bias;                                       /* (512,8192), (512)  */
    const float *fc2_weight, *fc2_bias;                                       /* (E,512), (E)       */
    const float *cls0_weight, *cls0_bias;                                     /* classifier.0: (64,E), (64) */
    const float *cls3_weight, *cls3_bias;                                     /* classifier.3: (1,64), (1)  */
    float bn_eps;                                                             /* 1e-5 (nn.BatchNorm2d default) */
} siggan_verifier_weights;

/* embedding_dim in 1..SIGGAN_VERIFIER_MAX_EMBEDDING; max_images >= 1 is the most images one call may carry (a score call
 * carries 2 * n_pairs).  The workspace (about 270 KB per image + 17 MB of packed weights) is allocated here, once. */
int siggan_verifier_create(int32_t device, int32_t embedding_dim, int32_t max_images, siggan_verifier **out);
int siggan_verifier_destroy(siggan_verifier *v);
/* Packs the conv / fc1 weights for the kernels and folds conv bias + BatchNorm into one scale / shift table per layer.
 * Call again whenever the weights change. */
int siggan_verifier_bind(siggan_verifier *v, const siggan_verifier_weights *w, void *stream);
/* x_dev: n_images images in `fmt` -> emb_dev (n_images, E), unit L2 norm per row */
int siggan_verifier_embed(siggan_verifier *v, const void *x_dev, int32_t fmt, int32_t n_images, float *emb_dev, void *stream);
/* e1_dev, e2_dev (n_pairs, E) -> score_dev (n_pairs): embed a gallery once, score it many times */
int siggan_verifier_compare(siggan_verifier *v, const float *e1_dev, const float *e2_dev, int32_t n_pairs, float *score_dev,
                            void *stream);
/* both images of every pair through the encoder as ONE batch of 2 * n_pairs images, then the head.  e1_dev / e2_dev may
 * be NULL when the embeddings are not wanted. */
int siggan_verifier_score(siggan_verifier *v, const void *x1_dev, const void *x2_dev, int32_t fmt, int32_t n_pairs,
                          float *e1_dev, float *e2_dev, float *score_dev, void *stream);
/* test hook: stage `name` ("pool1", "pool2", "pool3", "fc1") of the last embed / score call, in torch's layout (NCHW; fc1
 * as (N,512) after ReLU); n must be the stage's element count for that call's image count. */
int siggan_verifier_debug_tensor(siggan_verifier *v, const char *name, float *out_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_H */
