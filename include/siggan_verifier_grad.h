/*
 * siggan_verifier_grad.h -- C ABI of the Siamese signature verifier's eval-mode INPUT gradient on the MI355X: d objective /
 * d image through the network of siggan_verifier.h, on a siggan_verifier context (create / bind / destroy are that header's).
 * What generated signatures exist for is asked here: does the verifier take G(z) for the same hand as a target?  The image-space
 * gradient this call returns goes to siggan_g_latent_objective_grad_seeded (siggan.h), which carries it on to dz.
 *
 * Conventions are those of siggan_verifier.h.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 */
#ifndef SIGGAN_VERIFIER_GRAD_H
#define SIGGAN_VERIFIER_GRAD_H

#include "siggan_verifier.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- eval-mode input gradient: d objective / d image, BatchNorm as the folded affine of inference, no dropout ----
 * Per image b, against a constant reference embedding r[b] (siggan_verifier_embed of a target):
 *   objective[b] = embed_weight * 0.5 * sum_k (e[b,k] - r[b,k])^2  +  score_weight * -max(log s_b, -100),  s_b = head(e_b, r_b)
 * Images do not interact.  Rules: d(logit) of the score term is (s - 1) / max((1 - s) s, 1e-12) * s (1 - s); d|u|/du = sign(u)
 * with sign(0) = 0; F.normalize's backward is (de - e (e . de)) / max(||raw||, 1e-12); equal maxima of a pooling window route to
 * the first element in (dy, dx) order; ReLU passes only where the pre-activation is > 0.  A term whose weight is 0 contributes
 * nothing and is reported as 0.  Fixed-order sums, no atomics: equal inputs give equal bits.  16 launches on the caller's
 * stream (the embed call's five with the decisions recorded, head, embedding backward, the fc1 input gradient and per conv layer
 * an un-pool and an input gradient), no host synchronisation, capturable; weights and packs are untouched, the forward
 * workspace is rewritten as by siggan_verifier_embed. */
typedef struct siggan_verifier_identity {
    float embed_weight;   /* w_e >= 0, times 0.5 * sum_k (e[b,k] - r[b,k])^2   (= 1 - cos for unit rows)            */
    float score_weight;   /* w_s >= 0, times -max(log s_b, -100), s_b = head(e_b, r_b): BCE against "same writer" */
} siggan_verifier_identity;

/* Allocates the backward workspace for max_images, once; contexts that never call it pay nothing.  715332 + 5 E bytes per image
 * (about 0.70 MB: three route planes, dp1 and dy1, whose bytes first hold dp3 / dy3 / dp2 / dy2) + 500 KB of flipped conv packs,
 * which every later bind refreshes.  A set-up call: it may synchronise the device.  Calling it twice is a no-op. */
int siggan_verifier_input_grad_enable(siggan_verifier *v);

/* emb_dev is bit for bit siggan_verifier_embed(x_dev), score_dev bit for bit siggan_verifier_compare(emb, ref).  SIGGAN_E_ARG,
 * nothing enqueued: a null required pointer, a negative or non-finite weight or both 0, a misaligned x_dev / dx_dev, n_images
 * outside [1, max_images], a call before bind or before enable. */
int siggan_verifier_input_grad(siggan_verifier *v, const float *x_dev /* (N,1,64,64) fp32, 16-byte aligned */,
                               const float *ref_emb_dev /* (N,E): siggan_verifier_embed of the targets */, int32_t n_images,
                               const siggan_verifier_identity *w, float *dx_dev /* (N,1,64,64), required */,
                               float *objective_dev /* (N), required: w_e*embed + w_s*score */, float *terms_dev /* (2,N) optional, unweighted */,
                               float *score_dev /* (N) optional */, float *emb_dev /* (N,E) optional */, void *stream);

/* test hook, as siggan_verifier_train_debug: "route1|2|3" uint8 NCHW per pooled element (0..3 winner in (dy,dx) order, 4 = window
 * max not positive), "fc1_mask" (N,512), "cls_mask" (N,64) uint8, "diff_sign" (N,E) int8 in {-1,0,1}; of the last input_grad call */
int siggan_verifier_input_grad_debug(siggan_verifier *v, const char *name, void *out_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_VERIFIER_GRAD_H */
