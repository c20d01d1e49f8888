/*
 * siggan_shape.h -- C ABI of the shape attributes of a signature image on the MI355X: the ink moments up to second order
 * (how much ink, where it sits, how far it spreads, how it leans), a quadratic objective on them and that objective's gradient
 * with respect to the pixels, in fp64.  The gradient is an image-space seed for siggan_g_latent_objective_grad_seeded
 * (siggan.h), which carries it to the latent vector: that is how a generated signature is made to lean more, sit larger in
 * the frame, carry more ink or move off-centre.  A second call gives the same moments of byte images as exact integer sums.
 *
 * Both calls are context-free, like siggan_diverse.h: `device` is the HIP ordinal the pointers belong to.  Conventions are
 * those of siggan.h: plain pointers and sizes, a call enqueues on `stream` and never synchronises the host, it does not
 * allocate, it can be captured into a graph, 0 = OK / negative = SIGGAN_E_* with the message in siggan_last_error(), the
 * caller's current device is restored.  Adding this header did not change SIGGAN_ABI_VERSION: it only adds symbols.
 *
 * Definitions.  The image side is s = 64 or 128.  Pixel (row r, column c) has the coordinates u = (c + 0.5) / s - 0.5 and
 * v = (r + 0.5) / s - 0.5, both in (-0.5, 0.5) and exact in fp64; v grows DOWNWARDS.  The ink of an fp32 pixel x is
 * a = (1 - x) / 2, formed in fp64 and not clamped (x = +1 is paper, x = -1 full ink).  S0 = sum a; the image is EMPTY when
 * S0 <= 0.  The features f[0 .. 7] (SIGGAN_SHAPE_*):
 *   0 mass    S0 / s^2
 *   1 cx      sum a u / S0
 *   2 cy      sum a v / S0
 *   3 sxx     sum a (u - cx)^2 / S0
 *   4 syy     sum a (v - cy)^2 / S0
 *   5 sxy     sum a (u - cx)(v - cy) / S0
 *   6 slant   sxy / syy, or 0 when syy <= SIGGAN_SHAPE_SYY_MIN
 *   7 spread  sxx + syy
 * For an empty image f[1 .. 7] = 0.  The second moments are central sums formed in a second pass over the pixels with cx and
 * cy known, not raw moments minus squares.
 * Slant is the shear coefficient: shearing an image by x' = x + k y adds k to it.  Because v points down, a signature that
 * leans to the RIGHT ("/") has a NEGATIVE slant, one that leans to the left ("\") a positive one.
 *
 * Objective per image, with weights w[0 .. 7] and targets t[0 .. 7]:  obj = 1/2 sum_k w_k (f_k - t_k)^2.  Its gradient with
 * respect to pixel p is dx_p = -1/2 sum_k w_k (f_k - t_k) df_k/da_p (a = (1 - x) / 2), where with du = u_p - cx, dv = v_p - cy
 *   dmass = 1 / s^2,  dcx = du / S0,  dcy = dv / S0,  dsxx = (du^2 - sxx) / S0,  dsyy = (dv^2 - syy) / S0,
 *   dsxy = (du dv - sxy) / S0,  dslant = (dsxy - slant dsyy) / syy,  dspread = dsxx + dsyy
 * (the centre's own dependence on the pixels drops out of the central sums).  A feature with w_k == 0 is skipped and its
 * target is not looked at (it may be NaN).  On an empty image only the mass term contributes, and the slant term
 * contributes nothing when syy <= SIGGAN_SHAPE_SYY_MIN -- to the gradient and to the objective alike.  The kernel collects
 * the sum over k into the six coefficients of 1, du, dv, du^2, dv^2, du dv once per image and evaluates that polynomial per
 * pixel; dx is formed in fp64 and rounded once to fp32, the objective likewise.
 *
 * Arithmetic and order of the sums, fixed.  One launch, one workgroup of 256 lanes (four waves) per image, which reads its
 * image once, as 16-byte loads, and holds it in registers (16 or 64 floats per lane): lane l holds the pixels
 * 4 (256 j + l) + e, e = 0 .. 3, j = 0 .. s^2 / 1024 - 1 (p = r s + c).  Every sum is in fp64: each lane adds its terms in
 * ascending pixel order starting from 0.0 (terms: a, a * u, a * v; then a * (du * du), a * (dv * dv), a * (du * dv)), the 64
 * lane sums of a wave are folded by a butterfly, t = t + t(lane ^ o) for o = 32, 16, 8, 4, 2, 1, and the four wave sums are
 * folded through LDS in wave order, ((w0 + w1) + w2) + w3.  No fused multiply-add (the library is built with
 * -ffp-contract=off), no atomics; images do not interact: an image's outputs do not depend on the batch around it, and
 * equal input gives equal bits.
 */
#ifndef SIGGAN_SHAPE_H
#define SIGGAN_SHAPE_H

#include "siggan.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_SHAPE_FEATURES 8
#define SIGGAN_SHAPE_MASS     0
#define SIGGAN_SHAPE_CX       1
#define SIGGAN_SHAPE_CY       2
#define SIGGAN_SHAPE_SXX      3
#define SIGGAN_SHAPE_SYY      4
#define SIGGAN_SHAPE_SXY      5
#define SIGGAN_SHAPE_SLANT    6
#define SIGGAN_SHAPE_SPREAD   7
#define SIGGAN_SHAPE_SYY_MIN  1e-12     /* at or below it an image has no slant */
#define SIGGAN_SHAPE_SUMS     6         /* siggan_shape_u8: ink, ink p, ink q, ink p^2, ink q^2, ink p q */

/* x_dev (batch, 1, s, s) fp32, 16-byte aligned; weights_dev / targets_dev (batch, 8) fp64 or NULL; features_dev (batch, 8)
 * fp64, dx_dev (batch, 1, s, s) fp32 16-byte aligned, objective_dev (batch) fp32: each optional.  Outputs that overlap the
 * inputs are not part of the contract.
 * SIGGAN_E_INVALID with nothing enqueued: s not 64 or 128, batch < 1, a NULL or misaligned x_dev, a misaligned dx_dev, all
 * three outputs NULL, dx_dev or objective_dev given without both weights_dev and targets_dev, an fp64 pointer that is not
 * 8-byte aligned.
 * The weights live on the device and the call does not look at them: negative or non-finite weights are the caller's to
 * refuse (the Python layer does).  NaN / Inf pixels are not part of the contract. */
int siggan_shape_f32(int32_t device, const float *x_dev, int32_t batch, int32_t s, const double *weights_dev,
                     const double *targets_dev, double *features_dev, float *dx_dev, float *objective_dev, void *stream);

/* The statistics of byte images, exact: u8_dev (batch, s, s) uint8, 4-byte aligned; sums_dev (batch, 6) int64.  Ink is
 * 255 - b, the integer coordinates are p = 2 c + 1 - s and q = 2 r + 1 - s (u = p / (2 s), v = q / (2 s)), and the six raw sums
 * are sum ink, sum ink p, sum ink q, sum ink p^2, sum ink q^2, sum ink p q.  Nothing overflows: at s = 128 the largest sum is
 * below 6.8e10, and the products a host forms from them (S0 Spp - Sp^2) stay below 2.9e17.  Same launch shape, integers only:
 * a lane's 16 or 64 terms fit int32, the folds are int64.
 * SIGGAN_E_INVALID with nothing enqueued: s not 64 or 128, batch < 1, a NULL or misaligned u8_dev, a NULL sums_dev or one
 * that is not 8-byte aligned. */
int siggan_shape_u8(int32_t device, const uint8_t *u8_dev, int32_t batch, int32_t s, int64_t *sums_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_SHAPE_H */
