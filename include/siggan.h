/*
 * siggan.h -- C ABI of the MI355X (gfx950) signature-GAN engine.
 *
 * The reference (Nobita421/signature-Gan) has no FFI/plugin interface: its G+D train step and
 * its generation path sit behind Python classes.  This header is the boundary a maintainer
 * binds (ctypes) to route exactly that path to hand-written HIP kernels:
 *
 *   entry point              replaces (file:line under /root/reference/src)
 *   -----------------------  ---------------------------------------------------------------
 *   siggan_g_forward         Generator.forward            generator_vanilla_gan.py:189-209
 *                            (VanillaGAN.generate vanilla_gan_model.py:338-371,
 *                             generate_signatures_batch utils/inference.py:171-182)
 *   siggan_d_forward         Discriminator.forward / forward_features
 *                                                        discriminator_vanilla_gan.py:241-274
 *   siggan_d_step            VanillaGAN.train_discriminator_step vanilla_gan_model.py:180-252
 *                            == GANTrainer._train_discriminator  train_vanilla_gan_signatures.py:281-337
 *   siggan_g_step            VanillaGAN.train_generator_step    vanilla_gan_model.py:254-306
 *                            == GANTrainer._train_generator     train_vanilla_gan_signatures.py:339-376
 *   siggan_d_grads/_apply,   the same two steps cut at the point where a data-parallel run
 *   siggan_g_grads/_apply    averages the flat gradient bucket across ranks: with a communicator
 *                            (siggan_comm_init) *_apply itself issues the ncclAllReduce on the
 *                            step's stream ahead of the optimiser; without one, a host may reduce
 *                            the bound gradient arena between the two halves
 *   siggan_op_*              single kernels of the path (operator-level tests / profiling)
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer named *_dev is DEVICE memory of the context's
 *     GPU, fp32 unless stated; images are (B,1,S,S) contiguous (NCHW == NHWC for one channel).
 *   - ownership: the CALLER owns every tensor it passes (parameters, gradients, Adam moments,
 *     BatchNorm buffers, inputs, outputs) and their lifetime; the library owns only its
 *     workspace.  Parameter storage is BORROWED by siggan_bind: four flat arenas per network
 *     laid out in the reference's parameters() order, so the torch-side state_dict()/optimizer
 *     state stay authoritative and checkpoints need no conversion.
 *   - every call enqueues on `stream` (a hipStream_t passed as void*); no hidden device-wide
 *     synchronisation except where a HOST output pointer (metrics_host) is given.
 *   - return value: 0 = OK, negative = SIGGAN_E_*; never throws, never aborts.
 *     siggan_last_error() returns a thread-local message for the last failure.
 *   - one context per device per process; a context is not re-entrant.
 */
#ifndef SIGGAN_H
#define SIGGAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIGGAN_ABI_VERSION 4   /* 2: siggan_stage_real, siggan_augment_batch; 3: siggan_config.dtype, siggan_rng_state, siggan_comm_*;
                                * 4: siggan_config.g_leaky_slope (appended); siggan_prof_launch (a test hook, added);
                                *    siggan_g_generate_u8, siggan_image_stats (added: no existing call or struct changes);
                                *    siggan_d_score_u8, siggan_dequant_table (added likewise); siggan_g_latent_grad (added likewise);
                                *    siggan_g_latent_objective_grad with its struct siggan_latent_objective, added likewise;
                                *    siggan_g_param_grad, siggan_op_anchor (added likewise);
                                *    siggan_g_latent_objective_grad_seeded (added likewise) */

enum {
    SIGGAN_OK = 0,
    SIGGAN_E_INVALID = -1,     /* bad argument (maps to ValueError in the Python shim) */
    SIGGAN_E_STATE = -2,       /* call sequence / binding missing; a launch the library refused (sticky) */
    SIGGAN_E_HIP = -3,         /* HIP runtime error                                    */
    SIGGAN_E_NOMEM = -4
};

typedef struct siggan_ctx siggan_ctx;

/* Model geometry: Generator(latent_dim, output_size) / Discriminator(input_size)
 * (generator_vanilla_gan.py:97-121, discriminator_vanilla_gan.py:111-128). */
typedef struct siggan_config {
    int32_t device;         /* HIP device ordinal */
    int32_t latent_dim;     /* z dimension (reference default 100) */
    int32_t image_size;     /* 64 or 128 -- anything else is SIGGAN_E_INVALID (ValueError) */
    int32_t image_channels; /* only 1 (grayscale signatures) is built */
    int32_t max_batch;      /* largest per-call batch the workspace is sized for */
    float   dropout;        /* Discriminator dropout p (default 0.25) */
    float   leaky_slope;    /* LeakyReLU slope (default 0.2) */
    uint64_t seed;          /* seed of the library's counter-based RNG (z, dropout masks) */
    int32_t dtype;          /* SIGGAN_DTYPE_*: storage type of the library-owned activations / activation gradients and of
                             * the weight copies the MFMA kernels read.  F32 (0) is the reference's arithmetic and the parity
                             * path.  BF16 / F16 are build-defined narrow variants (BASELINE.json configs[2] / configs[4]; the
                             * reference has no reduced-precision mode, vanilla_gan_model.py:107-120): 16-bit storage, 16-bit
                             * MFMA operands, fp32 accumulation, fp32 master weights / BatchNorm statistics / losses / weight
                             * gradients / Adam.  Every caller-visible tensor stays fp32 in all modes. */
    float   f16_grad_scale; /* F16 only: power-of-two factor carried by the backward chains so that small activation
                             * gradients stay above the fp16 subnormals; removed again inside the optimiser step (the bound
                             * *_grads arenas hold scale x gradient between *_grads and *_apply).  0 = default (1024).
                             * The scale is STATIC (no dynamic loss scaling).  Protection against an overflow: in F16 mode
                             * *_apply takes the gradient arena's sum of squares first, and when it is not finite (an inf / NaN
                             * activation gradient reached a weight gradient) the whole update is SKIPPED -- parameters, moments
                             * and step counts untouched -- and SIGGAN_M_D_SKIPPED / SIGGAN_M_G_SKIPPED is set to 1 (else 0). */
    int32_t spectral_norm;  /* != 0: torch.nn.utils.spectral_norm on every Discriminator conv and on the classifier
                             * (Discriminator(use_spectral_norm=True), discriminator_vanilla_gan.py:60-62,200-202): the d_params
                             * arena then holds weight_orig, siggan_storage.d_sn_u / d_sn_v the weight_u / weight_v buffers; every
                             * training-mode Discriminator forward runs one power iteration (u, v updated in place), every forward
                             * divides the weights by sigma = u . (W v), and the D step's gradients flow through sigma. */
    float   g_leaky_slope;  /* the Generator's activation after every BatchNorm (fc block and upsample blocks).  0: ReLU, the
                             * reference Generator (generator_vanilla_gan.py:107-176).  > 0: LeakyReLU with this negative slope,
                             * the ablation study's ConfigurableGenerator(activation="leaky_relu", leaky_slope)
                             * (ablation_vanilla_gan_signatures.py:159-213 UpsampleBlockConfigurable, 216-328
                             * ConfigurableGenerator); the Discriminator's own LeakyReLU (leaky_slope above) is unaffected.  Must be
                             * finite and >= 0, else SIGGAN_E_INVALID.  Every mode, dtype, size and step variant supports it. */
} siggan_config;
enum { SIGGAN_DTYPE_F32 = 0, SIGGAN_DTYPE_BF16 = 1, SIGGAN_DTYPE_F16 = 2 };

/* Borrowed storage.  *_params / *_grads / *_exp_avg / *_exp_avg_sq: flat fp32 arenas holding
 * the network's parameters() in reference order (sizes: siggan_param_count).  *_adam_steps: one
 * fp32 per parameter TENSOR (torch.optim.Adam keeps `step` per tensor).  g_bn_*: BatchNorm
 * running statistics of all G BatchNorm layers concatenated in module order (fc.1, then
 * upsample_blocks.i.block.1); g_bn_batches: one int64 per BatchNorm layer. */
typedef struct siggan_storage {
    float *g_params, *g_grads, *g_exp_avg, *g_exp_avg_sq, *g_adam_steps;
    float *g_bn_running_mean, *g_bn_running_var;
    int64_t *g_bn_batches;
    float *d_params, *d_grads, *d_exp_avg, *d_exp_avg_sq, *d_adam_steps;
    /* spectral norm only (else NULL): weight_u of all layers (conv blocks in order, then the classifier) concatenated --
     * sizes Cout_l, 1 -- and weight_v likewise -- sizes Cin_l*16, 512*16 (siggan_sn_count) */
    float *d_sn_u, *d_sn_v;
} siggan_storage;

/* Optimiser / loss hyper-parameters of one step (vanilla_gan_model.py:60-72,
 * train_vanilla_gan_signatures.py:63-79). */
typedef struct siggan_hyper {
    double lr, beta1, beta2, eps; /* Adam, as the Python doubles torch.optim.Adam holds (eps: torch default
                                   * 1e-8); 1 - beta and the bias corrections are formed in double, as torch does */
    float label_smoothing;        /* real-label value in the D step (0.9) */
    float clip_max_norm;          /* <= 0: gradient clipping disabled */
    float grad_scale;             /* multiplies the gradients before clip/Adam (1/world for DP sums; 1 otherwise) */
} siggan_hyper;

/* metrics written by the step calls (fp32 each) */
enum {
    SIGGAN_M_D_LOSS = 0, SIGGAN_M_D_LOSS_REAL, SIGGAN_M_D_LOSS_FAKE, SIGGAN_M_D_REAL_MEAN,
    SIGGAN_M_D_FAKE_MEAN, SIGGAN_M_D_REAL_ACC, SIGGAN_M_D_FAKE_ACC, SIGGAN_M_D_GRAD_NORM,
    SIGGAN_M_G_LOSS, SIGGAN_M_G_FAKE_MEAN, SIGGAN_M_G_GRAD_NORM,
    SIGGAN_M_D_SKIPPED, SIGGAN_M_G_SKIPPED,    /* F16 only: 1 when the update was skipped for a non-finite gradient, else 0 */
    SIGGAN_M_COUNT = 16
};

/* ---- lifecycle ------------------------------------------------------------------------- */
int siggan_abi_version(void);
const char *siggan_last_error(void);
int siggan_create(const siggan_config *cfg, siggan_ctx **out);
int siggan_destroy(siggan_ctx *ctx);

/* which: 0 = generator, 1 = discriminator */
int64_t siggan_param_count(const siggan_ctx *ctx, int which);          /* scalars in the flat arena */
int32_t siggan_param_tensors(const siggan_ctx *ctx, int which);        /* number of parameter tensors */
/* offset (in floats) and element count of parameter tensor `idx` inside the flat arena */
int siggan_param_span(const siggan_ctx *ctx, int which, int32_t idx, int64_t *offset, int64_t *numel);
int64_t siggan_bn_count(const siggan_ctx *ctx);                        /* floats in g_bn_running_* */
int64_t siggan_sn_count(const siggan_ctx *ctx, int which);             /* floats in d_sn_u (which = 0) / d_sn_v (1) */
int32_t siggan_bn_layers(const siggan_ctx *ctx);
int64_t siggan_workspace_bytes(const siggan_ctx *ctx);

int siggan_bind(siggan_ctx *ctx, const siggan_storage *st);
/* tell the library the caller changed parameters / BN buffers / Adam step tensors behind its back
 * (load_state_dict, optimizer.load_state_dict, manual edits): packed weight copies are rebuilt on next
 * use, and the Adam step counts (which the library otherwise tracks on the host, so that an update is ONE
 * launch) are read back from *_adam_steps before the next *_apply */
int siggan_params_changed(siggan_ctx *ctx);
int siggan_seed(siggan_ctx *ctx, uint64_t seed, uint64_t offset);
/* reads the RNG position back (seed, call counter): a caller that re-creates a context (larger max_batch) or resumes a
 * run hands them to siggan_seed so the z / dropout stream continues instead of restarting; the reference's equivalent is
 * torch's global generator, which simply keeps running (train_vanilla_gan_signatures.py:313,356).  Synchronises. */
int siggan_rng_state(siggan_ctx *ctx, uint64_t *seed, uint64_t *offset);
/* execution mode of the step phases (default: SIGGAN_MODE_OVERLAP): SIGGAN_MODE_GRAPH replays each phase as a
 * hipGraph captured once per distinct (batch, flags, hyper-parameters); SIGGAN_MODE_OVERLAP runs
 * the weight-gradient / reduction kernels on side streams beside the input-gradient chain. */
#define SIGGAN_MODE_GRAPH 1
#define SIGGAN_MODE_OVERLAP 2
int siggan_set_mode(siggan_ctx *ctx, int32_t mode);

/* Which of the reference's two G+D iterations the step calls implement (default SIGGAN_STEP_TRAINER):
 *   TRAINER   GANTrainer._train_discriminator / _train_generator == VanillaGAN.train_*_step (train_vanilla_gan_signatures.py:
 *             281-376): D step with G in eval mode on its own z; G step with D in eval mode (no dropout), its own z, target 1.
 *   ABLATION  AblationGANTrainer.train_epoch (ablation_vanilla_gan_signatures.py:397-467): both nets stay in train mode; ONE
 *             Generator forward per iteration (BatchNorm batch statistics) whose detached output feeds the D update and
 *             through which the G update back-propagates; the G update's D pass draws fresh dropout masks and its target
 *             is the smoothed real label (hp->label_smoothing of siggan_g_grads).  Call order per iteration:
 *             siggan_d_grads(real, z, masks) -> siggan_d_apply -> siggan_g_grads(batch, z = NULL) -> siggan_g_apply; explicit
 *             masks are three sets (real pass, fake pass of the D update, fake pass of the G update). */
enum { SIGGAN_STEP_TRAINER = 0, SIGGAN_STEP_ABLATION = 1 };
int siggan_set_step_variant(siggan_ctx *ctx, int32_t variant);

/* ---- forward passes ---------------------------------------------------------------------- */
/* z_dev (B,latent) -> images_dev (B,1,S,S) in [-1,1].  training!=0: BatchNorm batch statistics,
 * running stats and num_batches_tracked updated (nn.Module.train()); 0: running stats (eval).
 * A training-mode Generator forward of ONE sample is refused with SIGGAN_E_INVALID and torch's text ("Expected more than 1
 * value per channel when training ...": the fc block's BatchNorm1d, generator_vanilla_gan.py:112) -- here, in siggan_g_grads
 * and in the ablation variant's siggan_d_grads; the trainer variant's D step accepts one sample (G.eval(), no BatchNorm in D),
 * and siggan_step_begin then does not start the Generator forward ahead of the siggan_g_grads that refuses it. */
int siggan_g_forward(siggan_ctx *ctx, const float *z_dev, int32_t batch, int32_t training,
                     float *images_dev, void *stream);

/* per-image stroke counters (int32 each): what the reference's calculate_stroke_density / calculate_foreground_ratio
 * (utils/metrics.py:118-174) count, for a pixel value t and a threshold thr, all in fp32:
 *   NEG         #{t < 0}                     -- summed over a batch it tells which branch the reference takes (images.min() < 0)
 *   INK_SIGNED  #{(t + 1.0f) * 0.5f < thr}   -- the branch for images in [-1, 1]
 *   INK_UNIT    #{t < thr}                   -- the branch for images in [0, 1]
 * A NaN pixel is not part of the contract. */
enum { SIGGAN_IS_NEG = 0, SIGGAN_IS_INK_SIGNED = 1, SIGGAN_IS_INK_UNIT = 2, SIGGAN_IS_COUNT = 3 };
/* Generator eval forward ending in what the callers of generation consume.  u8_dev (B,S,S) required (4-byte aligned): the
 * bytes of utils/inference.py:129, (t + 1) * 127.5 in fp32, clamped to [0, 255] and truncated;
 * images_dev (B,1,S,S) fp32 optional: bit-identical to siggan_g_forward(training = 0);
 * stats_dev (B, SIGGAN_IS_COUNT) int32 optional, zeroed by the call (threshold must then be finite). */
int siggan_g_generate_u8(siggan_ctx *ctx, const float *z_dev, int32_t batch, uint8_t *u8_dev,
                         float *images_dev, int32_t *stats_dev, float threshold, void *stream);

/* Eval-mode Generator forward of z_dev (B,latent), the per-image reconstruction loss against a target batch and its
 * gradient with respect to z: the primitive an optimiser on z runs around (projection of signatures into the latent space).
 * Exactly one of target_u8_dev (B,S,S) uint8 (4-byte aligned) and target_f32_dev (B,1,S,S) fp32 (16-byte aligned) is given; a
 * byte b stands for the fp32 value siggan_dequant_table gives it.
 *   loss_dev[b]   = mean over the S*S pixels of (x - t)^2,  x = G(z)[b]  (fp32)
 *   dz_dev[b, :]  = d loss_dev[b] / d z[b, :]               (eval mode: images do not interact)
 *   images_dev    optional (B,1,S,S), 16-byte aligned: bit for bit siggan_g_forward(training = 0)
 * fp32 contexts only.  Fixed-order sums, no atomics: equal inputs give equal bits.  A fixed sequence of launches on the
 * caller's stream, no host synchronisation.  It overwrites the Generator's activations (as siggan_g_forward does) and
 * training scratch no call carries over; a training step after it runs exactly as if it had not been called.  Refused with
 * SIGGAN_E_STATE between siggan_step_begin and its siggan_g_grads (the pipelined forward's activations are still needed). */
int siggan_g_latent_grad(siggan_ctx *ctx, const float *z_dev, int32_t batch, const uint8_t *target_u8_dev,
                         const float *target_f32_dev, float *dz_dev, float *loss_dev, float *images_dev, void *stream);

/* The gradient with respect to z of a per-image objective: what moves a latent vector towards images the Discriminator
 * believes (realism-guided refinement), towards a target (projection), and keeps it where the Generator was trained (prior). */
typedef struct siggan_latent_objective {
    float recon_weight;    /* w_r >= 0, times mean over pixels of (G(z) - t)^2        (needs a target)            */
    float realism_weight;  /* w_d >= 0, times -max(log D(G(z)), -100): BCE against 1, per image, D in eval mode  */
    float prior_weight;    /* w_p >= 0, times 0.5 * mean_k z[b,k]^2                                             */
} siggan_latent_objective;

/* Modes: Generator AND Discriminator run in eval mode -- Generator BatchNorm is its running-statistics affine, the
 * Discriminator has no dropout, and with spectral norm the weights are divided by sigma from the stored u, v, which do not move
 * (siggan_d_forward(training = 0)'s behaviour).  Images do not interact: every output row depends only on its own z row and
 * target.  The realism term and d(logit) use the G step's own expressions (BCE against 1 with the logarithm clamped at -100,
 * (p - 1) / max((1 - p) p, 1e-12) times p (1 - p)) with a count of 1 per image, not 1/B; d(logit) is multiplied by
 * realism_weight once.  A weight of 0 leaves that term's launches out: realism_weight == 0 runs no Discriminator kernel,
 * recon_weight == 0 reads no target.
 *   dz_dev (B,latent)      required: d objective[b] / d z[b,:]
 *   objective_dev (B)      required: w_r*recon + w_d*realism + w_p*prior, in that order
 *   terms_dev (3,B)        optional: the unweighted recon, realism, prior terms; a term whose weight is 0 is written as 0
 *   probs_dev (B)          optional: D(G(z)); requires realism_weight > 0
 *   images_dev (B,1,S,S)   optional, 16-byte aligned
 * Refused with SIGGAN_E_INVALID, nothing enqueued: a negative or non-finite weight; all three weights 0; recon_weight > 0
 * without exactly one target; recon_weight == 0 with a target; probs_dev with realism_weight == 0; a target or images_dev
 * that breaks the alignment rules of siggan_g_latent_grad; a 16-bit context.  SIGGAN_E_STATE between siggan_step_begin and
 * its siggan_g_grads, as siggan_g_latent_grad.
 * Bits: siggan_g_latent_grad IS this call with the weights (1, 0, 0) -- one device sequence, its loss_dev in objective_dev's
 * place, no terms and no probs -- so the two give the same dz, loss and images; images_dev is bit for bit siggan_g_forward(training = 0); probs_dev is bit for bit what siggan_d_forward(training = 0)
 * returns for images_dev at the same batch size; byte and fp32 targets holding the same values give the same bits; two calls
 * on equal inputs give equal bits (fixed-order sums, no atomics).
 * A fixed sequence of launches on the caller's stream, no host synchronisation.  Training state, RNG, BatchNorm buffers and
 * u, v are untouched; the context is left as a siggan_g_latent_grad followed by a siggan_d_forward(training = 0) would leave it
 * (realism_weight == 0: as siggan_g_latent_grad alone), and a train step after it, eager or captured, runs exactly as if it had
 * not been called. */
int siggan_g_latent_objective_grad(siggan_ctx *ctx, const float *z_dev, int32_t batch, const uint8_t *target_u8_dev,
                                   const float *target_f32_dev, const siggan_latent_objective *w, float *dz_dev,
                                   float *objective_dev, float *terms_dev, float *probs_dev, float *images_dev, void *stream);

/* siggan_g_latent_objective_grad plus <image_grad[b], G(z)[b]> linearised: dz[b,:] additionally receives J_G(z_b)^T image_grad[b]
 * -- the call becomes a general vector-Jacobian product of the eval-mode Generator (an identity term from the verifier's
 * siggan_verifier_input_grad on 64x64 contexts, or any image-space loss the caller owns).
 * image_grad_dev (B,1,S,S) fp32, 16-byte aligned, required (use the unseeded call otherwise).  With a seed all three weights may be 0:
 * objective_dev is then written as 0.  objective / terms / probs / images never include the seed's term -- the caller owns that loss.
 * The seed joins d(pre-tanh) behind the Discriminator's and the reconstruction's seeds, in that order: fmaf(seed, 1 - x^2, dpre),
 * or seed * (1 - x^2) when nothing is there yet (one more launch); everything downstream is the unseeded call's chain, so a zero
 * seed gives the unseeded call's bits.  Refusals (plus a null or misaligned image_grad_dev; minus "all three weights 0"),
 * SIGGAN_E_STATE and the "training state untouched" contract are those of siggan_g_latent_objective_grad. */
int siggan_g_latent_objective_grad_seeded(siggan_ctx *ctx, const float *z_dev, int32_t batch, const uint8_t *target_u8_dev,
        const float *target_f32_dev, const siggan_latent_objective *w, const float *image_grad_dev, float *dz_dev,
        float *objective_dev, float *terms_dev, float *probs_dev, float *images_dev, void *stream);

/* The gradient with respect to the Generator's PARAMETERS of the same per-image objective, summed over the batch: what adapts
 * the model to a handful of target signatures (pivotal tuning: hold the projected latents fixed, run Adam on the weights).
 * obj_b = w_r * mean((G(z_b) - t_b)^2) + w_d * -max(log D(G(z_b)), -100), both networks in eval mode, the expressions, the
 * byte dequantisation and the count of 1 per image of siggan_g_latent_objective_grad; prior_weight must be 0 (the prior does
 * not depend on the parameters).  BatchNorm is the fixed per-channel affine of its running statistics: one sample is fine,
 * nothing moves, dbeta[c] = sum dpost, dgamma[c] = sum dpost * xhat with xhat from the pre-BatchNorm tensor and the running
 * statistics -- right for gamma of either sign and for gamma == 0 -- and no batch-correction terms.
 *   dparams_dev            required, 16-byte aligned, caller-owned (NOT the bound g_grads): siggan_param_count(ctx, 0) floats
 *                          in the arena's layout (siggan_param_span); receives sum_b d obj_b / d theta -- pass grad_scale = 1/B
 *                          to siggan_op_adam for the mean
 *   first_layer            0 .. Lg + 1 (Lg = siggan_bn_layers(ctx) - 1 blocks).  Layer 0: fc.0.{weight,bias}, fc.1.{weight,bias};
 *                          layer l = 1 .. Lg: upsample_blocks.{l-1} (ConvT weight, BatchNorm weight, bias); layer Lg + 1:
 *                          final_conv.0.{weight,bias}.  Tensors of layers >= first_layer get their gradient, the spans below
 *                          are written as 0, and the backward chain stops where it is no longer needed (Lg + 1: no block GEMM;
 *                          l: the input-gradient GEMMs of blocks Lg .. l + 1 only)
 *   objective_dev (B)      optional;  terms_dev (3,B) optional, the prior row written as 0;  probs_dev (B) optional, requires
 *                          realism_weight > 0;  images_dev (B,1,S,S) optional, 16-byte aligned
 * Refused with SIGGAN_E_INVALID, nothing enqueued: what siggan_g_latent_objective_grad refuses, prior_weight != 0, both
 * weights 0, first_layer out of range, a null or misaligned dparams_dev.  SIGGAN_E_STATE between siggan_step_begin and its
 * siggan_g_grads.
 * Bits: fixed-order sums, no float atomics -- two calls on equal inputs give equal bits; byte and fp32 targets holding the same
 * values give the same bits; the trainable spans do not depend on first_layer.  The forward keeps every block's pre-BatchNorm
 * tensor (raw GEMM, then the eval affine as its own launch); images, objective, terms and probs are those of
 * siggan_g_latent_objective_grad to within the README's forward tolerance (the same expression on the same accumulators).
 * A fixed sequence of launches on the caller's stream, no host synchronisation, capturable.  Parameters, Adam state, the RNG,
 * the BatchNorm running tensors and counters and u, v are untouched; a train step after it, eager or captured, runs exactly as
 * if it had not been called. */
int siggan_g_param_grad(siggan_ctx *ctx, const float *z_dev, int32_t batch, const uint8_t *target_u8_dev,
                        const float *target_f32_dev, const siggan_latent_objective *w, int32_t first_layer,
                        float *dparams_dev, float *objective_dev, float *terms_dev, float *probs_dev, float *images_dev,
                        void *stream);

/* x_dev (B,1,S,S) -> probs_dev (B) probabilities.  features_dev (B,512*4*4, reference
 * flatten order c,h,w) optional.  training!=0 enables Dropout2d: masks_dev, if given, holds the
 * keep masks (1 keep / 0 drop) of all blocks concatenated [(B,C_1),(B,C_2),...]; NULL draws
 * them from the library RNG. */
int siggan_d_forward(siggan_ctx *ctx, const float *x_dev, int32_t batch, int32_t training,
                     const float *masks_dev, float *probs_dev, float *features_dev, void *stream);

/* Eval-mode Discriminator forward from the bytes generation ends in (siggan_g_generate_u8): the scoring step of the reference
 * app's "Filter by Realism" (app_vanilla_gan_signatures.py:1364-1372).  u8_dev (B,S,S) uint8.  binarize -1: off; 0..255: a byte b
 * becomes b < binarize ? 0 : 255 first (process_images, :863-904).  The first block dequantises on load, t = b / 127.5 - 1.0
 * as the reference's fp32 expression on the CPU gives it (a correctly rounded division, then a subtraction: the values of
 * siggan_dequant_table); the zero padding is 0.0f in that domain.  probs_dev (B) is bit for bit what
 * siggan_d_forward(training = 0) gives for that fp32 tensor, which x_dev (optional, (B,1,S,S) fp32) receives; the call
 * enqueues the launches of siggan_d_forward, no more, and leaves the context as that call does. */
int siggan_d_score_u8(siggan_ctx *ctx, const uint8_t *u8_dev, int32_t batch, int32_t binarize, float *probs_dev,
                      float *x_dev, void *stream);
/* table_host[b], b in 0..255 (HOST memory): the fp32 value siggan_d_score_u8 gives byte b.  Needs no context and no device. */
int siggan_dequant_table(float *table_host);

/* ---- training steps ---------------------------------------------------------------------- */
/* D step: D(real) vs label_smoothing, G_eval(z) under no-grad, D(fake) vs 0, backward into D,
 * optional clip, Adam(D).  z_dev NULL: z ~ N(0,1) from the library RNG.  masks_dev NULL: library
 * RNG; else keep masks for the real pass then the fake pass, each [(B,C_1)...(B,C_n)].
 * metrics_dev (SIGGAN_M_COUNT floats, optional) receives the metrics on the device;
 * metrics_host (optional) additionally copies them to the host and synchronises the stream. */
int siggan_d_step(siggan_ctx *ctx, const float *real_dev, int32_t batch, const float *z_dev,
                  const float *masks_dev, const siggan_hyper *hp, float *metrics_dev,
                  float *metrics_host, void *stream);
/* G step: G_train(z) (BN batch stats + running-stat update), D_eval(fake), BCE vs 1.0, backward
 * through D into G (D weight gradients are not formed), optional clip, Adam(G). */
int siggan_g_step(siggan_ctx *ctx, int32_t batch, const float *z_dev, const siggan_hyper *hp,
                  float *metrics_dev, float *metrics_host, void *stream);

/* ---- data parallelism: one process per GPU, per-replica BatchNorm, ONE sum all-reduce of the flat
 * gradient bucket per network per step over RCCL (xGMI), issued INSIDE siggan_d_apply / siggan_g_apply -- hence inside
 * siggan_d_step / siggan_g_step -- once a communicator exists.  The reference is single-process (no torch.distributed
 * anywhere); this is the definition SURVEY 8(e) fixes: every rank runs the reference's step (train_vanilla_gan_signatures.py:
 * 281-376) on its contiguous shard of the global batch, gradients are averaged (the optimiser multiplies the summed bucket by
 * grad_scale / world), clipping acts on the averaged gradient, metrics stay per rank.
 *   siggan_comm_unique_id  rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks by any channel the
 *                          launcher has (a file, MPI, a TCP store; the Python shim uses torch.distributed's store once)
 *   siggan_comm_init       every rank, same id: ncclCommInitRank on the context's device.  world == 1 is allowed (the
 *                          all-reduce then runs and changes nothing) -- used by the single-GPU tests
 *   siggan_comm_broadcast  root's bytes to every rank (initial parameters / optimiser state), in place
 * RCCL is resolved at run time from the copy the process already holds (torch's), see siggan.hip; the library owns the
 * communicator and destroys it with the context.  Not available under SIGGAN_MODE_GRAPH. */
#define SIGGAN_COMM_ID_BYTES 128
int siggan_comm_unique_id(void *id_out);
int siggan_comm_init(siggan_ctx *ctx, int32_t rank, int32_t world, const void *id);
int siggan_comm_destroy(siggan_ctx *ctx);
int32_t siggan_comm_world(const siggan_ctx *ctx);   /* 1 without a communicator */
int siggan_comm_broadcast(siggan_ctx *ctx, void *buf_dev, int64_t bytes, int32_t root, void *stream);

/* step halves: *_grads leaves the local gradient in the bound *_grads arena (and the forward metrics in metrics_dev);
 * *_apply (all-reduces the arena when a communicator exists, then) scales by hp->grad_scale (/ world), clips and runs
 * Adam.  Without a communicator a caller may reduce the arena itself between the halves (the gloo tests do). */
int siggan_d_grads(siggan_ctx *ctx, const float *real_dev, int32_t batch, const float *z_dev,
                   const float *masks_dev, const siggan_hyper *hp, float *metrics_dev, void *stream);
/* siggan_d_grads that ALSO enqueues the following G step's training forward (z: zg_dev, or the library
 * RNG when NULL) on its own lane beside the D step's backward -- that forward depends on nothing the D
 * step changes (train_vanilla_gan_signatures.py:349-357).  Must be followed by siggan_d_apply and then
 * siggan_g_grads(batch, z_dev = NULL), which picks the forward up.  Results are bit-identical to the
 * un-pipelined calls; without SIGGAN_MODE_OVERLAP it degrades to siggan_d_grads.
 * With a communicator this call (like siggan_d_step, and unlike siggan_d_grads, which never starts a collective) already
 * issues the all-reduce of the last Discriminator block's weight gradient -- three quarters of the D bucket, complete first
 * -- on a lane of its own under the rest of the backward pass; siggan_d_apply reduces the remainder and waits for it.  EVERY
 * rank must therefore follow it with siggan_d_apply. */
int siggan_step_begin(siggan_ctx *ctx, const float *real_dev, int32_t batch, const float *z_dev,
                      const float *masks_dev, const float *zg_dev, const siggan_hyper *hp,
                      float *metrics_dev, void *stream);
/* Software-pipelining across steps: hands the library the real batch of the NEXT D step (BORROWED, not
 * copied: real_dev must stay valid and unmodified until the siggan_d_grads / siggan_step_begin that consumes
 * it has returned -- that call copies it into the workspace; the loop of GANTrainer.train_epoch,
 * train_vanilla_gan_signatures.py:378-405, knows the batch one iteration early and its loader keeps it alive).  Call it after siggan_d_apply and before siggan_g_grads: that siggan_g_grads then
 * runs the staged batch's D(real) forward (discriminator weights are final by then) on its own lane beside
 * the Generator backward.  The next siggan_d_grads / siggan_step_begin consumes the staged batch when
 * called with real_dev = NULL (a non-NULL real_dev discards it).  Results are bit-identical to the
 * un-staged sequence as long as exactly one siggan_g_apply lies in between; without SIGGAN_MODE_OVERLAP
 * (or under graph replay) the staged batch is simply used as the real batch. */
int siggan_stage_real(siggan_ctx *ctx, const float *real_dev, int32_t batch, void *stream);
int siggan_d_apply(siggan_ctx *ctx, const siggan_hyper *hp, float *metrics_dev, float *metrics_host,
                   void *stream);
int siggan_g_grads(siggan_ctx *ctx, int32_t batch, const float *z_dev, const siggan_hyper *hp,
                   float *metrics_dev, void *stream);
int siggan_g_apply(siggan_ctx *ctx, const siggan_hyper *hp, float *metrics_dev, float *metrics_host,
                   void *stream);

/* ---- operator-level entry points (tests, profiling) --------------------------------------- */
/* Activation tensors NHWC on the device in the CONTEXT's element type (fp32, or bf16 / f16 for a narrow context);
 * weights and weight gradients always fp32 in the reference's layouts.  4x4 stride-2 pad-1 convolution family on MFMA:
 *   form 0 "down": out[n,oh,ow,co] = sum_{kh,kw,ci} in[n,2oh-1+kh,2ow-1+kw,ci] * w[co,ci,kh,kw]
 *                  (Conv2d forward; ConvTranspose2d input-gradient)            w is (Cout,Cin,4,4)
 *   form 1 "up"  : out[n,oh,ow,co] = sum_{ci,kh,kw: oh=2ih-1+kh} in[n,ih,iw,ci] * w[ci,co,kh,kw]
 *                  (ConvTranspose2d forward; Conv2d input-gradient)            w is (Cin,Cout,4,4)
 * w_dev is in the reference's (torch) layout; the library packs it. */
int siggan_op_conv4x4s2(siggan_ctx *ctx, int32_t form, const void *in_dev, const float *w_dev,
                        void *out_dev, int32_t batch, int32_t h_in, int32_t c_in, int32_t c_out,
                        void *stream);
/* weight gradient of the same family: dw[cs,cl,kh,kw] = sum_{n,p,q} small[n,p,q,cs] *
 * large[n,2p-1+kh,2q-1+kw,cl]; dw_dev in torch layout (Cs,Cl,4,4). */
int siggan_op_conv4x4s2_wgrad(siggan_ctx *ctx, const void *small_dev, const void *large_dev,
                              float *dw_dev, int32_t batch, int32_t h_small, int32_t c_small,
                              int32_t c_large, void *stream);
/* fused Adam over a flat arena (torch.optim.Adam single step, step = count AFTER increment) */
int siggan_op_adam(siggan_ctx *ctx, float *p_dev, float *g_dev, float *m_dev, float *v_dev,
                   int64_t n, int32_t step, const siggan_hyper *hp, void *stream);
/* g[i] += weight * (p[i] - p0[i]), i < n: the gradient of 0.5 * weight * |p - p0|^2 (an anchor to a snapshot p0 of the
 * parameters, the regulariser of few-shot adaptation).  Any n >= 1; weight finite and >= 0; three separately rounded fp32
 * operations per element. */
int siggan_op_anchor(siggan_ctx *ctx, float *g_dev, const float *p_dev, const float *p0_dev, int64_t n, float weight,
                     void *stream);
/* library RNG: n standard normals / n Bernoulli(keep) keep-masks */
int siggan_op_randn(siggan_ctx *ctx, float *out_dev, int64_t n, void *stream);
/* Input pipeline (replaces SignatureDataset.__getitem__ + the transform chain of
 * get_train_transforms / get_val_transforms, data_loader_signatures.py:107-138,153-243, for a whole batch):
 * out[b] = Normalize(ToTensor(hflip?(RandomAffine_scale(RandomRotation(cache[index[b]])))))  as (batch,1,size,size)
 * fp32 in HBM, from an (N,size,size) uint8 cache of decoded + resized images resident in HBM.  Needs no context.
 *   params_dev [batch][8] int32: {mode, a0, a1, a2, a3, a4, a5, flags} -- rotation stage: mode 0 = copy, 1 = Pillow's
 *     16.16 fixed-point affine (output (x,y) samples input ((a2 + y*a1 + x*a0) >> 16, (a5 + y*a4 + x*a3) >> 16)),
 *     2 = per-axis tables (rows 0,1 of tables_dev); flags bit 0: horizontal flip, bit 1: scale stage present
 *   tables_dev [batch][4][size] int16: source column / row per output column / row (-1 = outside -> fill); rows 2,3 are
 *     the scale stage (Pillow's ImagingScaleAffine positions, tabulated by the host in double precision)
 *   lut_dev [256] fp32: value of each byte after ToTensor + Normalize;  augment = 0: out[b] = lut[cache[index[b]]].
 * The host side (signature-gan_amd/data_loader_signatures.py) draws indices, angles and scales with the reference
 * DataLoader's own RNG protocol and fills params / tables. */
int siggan_augment_batch(int32_t device, const uint8_t *cache_dev, int64_t n_images, const int32_t *index_dev,
                         const int32_t *params_dev, const int16_t *tables_dev, const float *lut_dev,
                         float *out_dev, int32_t batch, int32_t size, int32_t augment, int32_t fill,
                         void *stream);
/* the same counters for any fp32 image tensor x_dev (batch, pixels) on `device`, pixels any positive count; stats_dev
 * (batch, SIGGAN_IS_COUNT) int32 is zeroed by the call.  Needs no context. */
int siggan_image_stats(int32_t device, const float *x_dev, int32_t batch, int64_t pixels,
                       float threshold, int32_t *stats_dev, void *stream);
/* what the roofline peaks are derived from (bench.py): compute units x shader clock (kHz) of the device, and its HBM size */
int siggan_device_info(int32_t device, int32_t *compute_units, int32_t *clock_khz, int64_t *hbm_bytes);
/* measurement hook (bench.py roofline leg): while enabled, every MFMA implicit-GEMM launch is
 * bracketed by HIP events on the stream it is launched on.  siggan_prof_read synchronises the
 * device and returns, for kernel slot idx (0..siggan_prof_slots()-1): its name, launch count,
 * summed device time (ms), summed algorithmic FLOPs and summed algorithmic HBM bytes (operands read once + result
 * written once, in the context's element type). */
int siggan_prof_enable(siggan_ctx *ctx, int32_t on);
int32_t siggan_prof_slots(void);
int siggan_prof_read(siggan_ctx *ctx, int32_t idx, char *name, int32_t name_cap, int64_t *launches,
                     double *ms, double *flops, double *bytes);
/* test hook: *count = the launches recorded since siggan_prof_enable; for launch idx (in launch order) the first n of
 * {kernel slot, form (0 down / 1 up), epilogue asked for, epilogue run, rows per class M, Ci, Co, K slabs (> 1: summed and
 * finished by the split-K epilogue kernel), in-workgroup K split (1 or 2)} (gconv.h: GConvArgs, enum Epilogue; -1 where a
 * launch is no implicit GEMM).  Does not synchronise. */
int siggan_prof_launch(siggan_ctx *ctx, int64_t idx, int32_t *fields, int32_t n, int64_t *count);

/* test hook: copy the first n elements of a library-owned workspace tensor (NHWC), converted to fp32, into out_dev:
 * "g_y"/"g_a"/"g_da" (layer 0..Lg), "d_a"/"d_dv" (block 1..Ld), "img", "dpre", "logits",
 * "probs", "dlogit"; "d_noise" (block 1..Ld): the dropout multipliers (0 or 1/keep) of the last D step, [2B][C_l] -- rows
 * [0, B) the D(real) pass, [B, 2B) the D(fake) pass.  Scalars (n = 1, index 0; the call synchronises the stream):
 * "rode" -- the batch whose first Discriminator block the last siggan_g_grads took from the riders of the preceding D
 * update (0: it ran the block itself); "pre_real" -- the batch whose D(real) forward that call started ahead beside the
 * Generator backward (siggan_stage_real; 0: none); "ride_late" -- 1 once an update's riders did not report in time (sticky:
 * every later step call returns SIGGAN_E_STATE).  Used by tests that localise a parity failure. */
int siggan_debug_tensor(siggan_ctx *ctx, const char *name, int32_t index, float *out_dev, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGGAN_H */
