"""Shared by the latent-objective and refinement tests (and profiles/latent_objective_parity_margins.py): the fp64 oracle side of
the per-image objective  w_r * mean((G(z) - t)^2) + w_d * -log D(G(z)) + w_p * 0.5 * mean(z^2)  through the eval-mode Generator
and the eval-mode Discriminator, and the engines the device side runs on."""
import numpy as np
import torch
import torch.nn.functional as F

from common import I, O, SEED, oracle_states, oracle_states_sn
from latentcommon import P_BETAS, P_LATENT, P_SIZE, oracle_sd64

GAIN = {64: 32.0, 128: 16.0}       # the final-conv gain of test_latent_grad_gpu: the images span the range and saturate in places
#        S   latent B  G slope  spectral norm
CASES = [(64, 100, 3, 0.0, False),       # ragged GEMM rows in both networks
         (64, 100, 1, 0.0, False),       # the Discriminator's last block has 16 rows
         (128, 128, 2, 0.0, False),      # five blocks per network
         (64, 50, 2, 0.0, False),        # generic fc kernels
         (64, 100, 2, 0.2, False),       # LeakyReLU Generator
         (64, 100, 2, 0.0, True)]        # W / sigma from the stored u, v
# realism alone; all three (16 brings the reconstruction gradient to the realism gradient's order at 64x64, so an error in
# either is visible); reconstruction alone
WEIGHTS = [(0.0, 1.0, 0.0), (16.0, 1.0, 0.5), (1.0, 0.0, 0.0)]
# The batches the callers run (project_signatures, refine_latents, edit_latents, adapt_generator work in chunks of the engine's
# max_batch, 64 by default), each the smallest that reaches its launcher paths: (case, z seed).  What each reaches is
# evalpaths.describe(size, latent, batch), held to the sources by test_eval_paths_cpu.py and to the library's launch profile by
# test_eval_grad_batches_gpu.py.  The Generator's chains are 256-128-64-32-32 and 512-256-128-64-32-32 (siggan.hip).
BATCH_CASES = [
    # k_fc_dz's second image tile with one live row; three objective workgroups, the last a single wave; the first scale table
    # copied by two workgroups; k_bn_eval_bwd on block 1 in two chunks, the second 64 rows; every GEMM still slab-split
    ((64, 100, 9, 0.0, False), SEED["z"]),
    # generic fc kernels (latent % 4 != 0), one k pass in k_fc_dz, a second tile with 5 live rows, the LeakyReLU variants; the
    # Discriminator chain's five- and three-way slab splits
    ((64, 50, 13, 0.2, False), SEED["z"]),
    # the default chunk: l = 4 as unsplit k_gconv<128,32> (512 workgroups) and l = 3 as the two-quad k_gconv<64,64>, both with
    # EPI_LRELU_BWD and the scale table in the kernel; l = 2 as a 4-slab split; the Discriminator's chain without slabs (l = 4
    # two-quad)
    ((64, 100, 64, 0.0, False), SEED["z"]),
    # l = 5 as unsplit k_gconv<128,32> at exactly 384 workgroups; l = 4 as a three-way, l = 3 as a six-way slab split; k_fc_dz's
    # second tile with 4 live rows.  (At SEED["z"], +3, +7, +8 the fp64 oracle's logits reach 6.5 .. 10.8: this z keeps them < 6)
    ((128, 128, 12, 0.0, False), SEED["z"] + 2),
    # l = 3 and l = 2 as unsplit one-quad k_gconv<64,64> with the table in the kernel, l = 1 two-quad; the Discriminator's l = 3
    # as k_gconv<128,128>; 32 image tiles in k_fc_dz, 64 objective workgroups, table copies of 32 / 16 / 8 workgroups
    ((64, 100, 256, 0.0, False), SEED["z"]),
    # launch_fc_dz halves nsplit once B * latent exceeds 32767 at 64x64 (64 * B * latent > PARTIAL_FLOATS - 64): 64 images at
    # latent 512 are the smallest batch of whole tiles that does -- nsplit 32, so every k_fc_dz workgroup walks TWO 64-feature
    # chunks (the f0 loop with its barriers), in eight passes over k and eight image tiles; the GEMMs are those of B = 64
    ((64, 512, 64, 0.0, False), SEED["z"]),
]

R_STEPS, R_LR = 20, 0.02           # the refinement loop of test_refine_gpu


def oracle_d_sd64(size, uv=None):
    """The synthetic Discriminator state in fp64 as the eval-mode forward runs it.  ``uv``: the (u, v) dict of a
    spectral-norm context -- every weight is then weight_orig / sigma from these vectors (sn_weights(training=False): they do
    not move)."""
    d64 = {k: v.double() for k, v in oracle_states(size, 100, warm=False)[1].items()}
    if uv is None:
        return d64
    return O.sn_weights(d64, {k: v.double().cpu() for k, v in uv.items()}, size, training=False)


def oracle_objective(g_sd64, d_sd64, z, t64, size, signs_g=None, signs_d=None, slope=0.0, rec_g=None, rec_d=None,
                     dtype=torch.float64):
    """The three unweighted terms (3, B), their gradients with respect to z (3, B, latent) and the logits (B,) in fp64.
    ``signs_*``: another implementation's activation decisions in the two networks (None: the run's own); ``t64`` None: no
    reconstruction term (zeros).  The objective is linear in the terms, so one run serves every weight set.  ``dtype``: the
    type z is run in -- torch.float32 with states and target cast alike is torch's own fp32 arithmetic, the yardstick for how
    well conditioned a z is."""
    z64 = z.to(dtype).clone().requires_grad_()
    img = O.g_forward(g_sd64, z64, False, size, signs=signs_g, record=rec_g, slope=slope)
    feat = O.d_features(d_sd64, img, size, None, signs=signs_d, record=rec_d)
    logit = F.linear(feat, d_sd64["classifier.0.weight"], d_sd64["classifier.0.bias"])[:, 0]
    recon = ((img[:, 0] - t64) ** 2).mean(dim=(1, 2)) if t64 is not None else 0.0 * z64.sum(dim=1)
    terms = [recon, F.softplus(-logit), 0.5 * (z64 ** 2).mean(dim=1)]          # -log sigmoid(x) = softplus(-x)
    grads = [torch.autograd.grad(t.sum(), z64, retain_graph=True)[0] for t in terms]
    return torch.stack([t.detach() for t in terms]), torch.stack(grads), logit.detach()


def combine(w, parts):
    """w_r * parts[0] + w_d * parts[1] + w_p * parts[2] in fp64."""
    return sum(float(wi) * p for wi, p in zip(w, parts))


def objective_engine(size, latent, batch, slope=0.0, sn=False, dtype="f32", gain=None):
    """An Engine on the cold synthetic state of oracle_states (the spectral-norm case: the synthetic u, v after eight power
    iterations), the final conv multiplied by ``gain`` (default GAIN[size])."""
    from hipcommon import load_engine_state
    from signature_gan_amd.engine import Engine
    kw = dict(g_activation="leaky_relu", g_leaky_slope=slope) if slope else {}
    eng = load_engine_state(Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", seed=0, dtype=dtype,
                                   spectral_norm=sn, **kw), size, latent, False)
    if sn:
        # the synthetic weight_u / weight_v are random directions, whose sigma is far below the spectral norm: the weights
        # divided by it put every logit near -1e7 (fp64 oracle) and saturate every score.  Eight power iterations
        # (train()-mode forwards, as test_d_score_u8_gpu does) bring sigma to the spectral norm, where the scores spread; the
        # oracle then runs on the vectors read back from the context (Engine.sn_views), which the call under test must not move.
        uv = oracle_states_sn(size, latent)[4]
        for k, v in eng.sn_views().items():
            v.copy_(uv[k])
        x = torch.from_numpy(I.gen_real(batch, size, SEED["real"])).cuda()
        for _ in range(8):
            eng.d_forward(x, training=True)
    g = GAIN[size] if gain is None else gain
    v = eng.views("g")
    v["final_conv.0.weight"].mul_(g); v["final_conv.0.bias"].mul_(g)
    eng.params_changed()
    return eng


def hip_signs_d_rows(eng, size, batch):
    """The Discriminator's activation decisions in workspace rows [0, batch), NCHW bool per block (as after siggan_d_forward)."""
    out = []
    for l, c in enumerate(list(O.D_CHAIN[size]), start=1):
        h = size >> l
        out.append(eng.debug_tensor("d_a", l, (batch, h, h, c)).permute(0, 3, 1, 2).contiguous().cpu() > 0)
    return out


def oracle_refine(z0, steps, lr, realism_weight=1.0, prior_weight=0.0):
    """refine_latents' loop on the CPU: the oracle in fp64 under torch.optim.Adam on the projection case's cold state (no
    gain).  Returns (the (steps, N) objective history -- the objective at the start of every iteration --, the (steps, N)
    logits, the final z)."""
    g64, d64 = oracle_sd64(P_SIZE, P_LATENT), oracle_d_sd64(P_SIZE)
    z = z0.double().clone().requires_grad_()
    opt = torch.optim.Adam([z], lr=lr, betas=P_BETAS)
    hist, logits = [], []
    for _ in range(steps):
        opt.zero_grad()
        img = O.g_forward(g64, z, False, P_SIZE)
        logit = F.linear(O.d_features(d64, img, P_SIZE, None), d64["classifier.0.weight"], d64["classifier.0.bias"])[:, 0]
        obj = realism_weight * F.softplus(-logit) + prior_weight * 0.5 * (z ** 2).mean(dim=1)
        obj.sum().backward()
        hist.append(obj.detach().clone()); logits.append(logit.detach().clone())
        opt.step()
    return torch.stack(hist), torch.stack(logits), z.detach()


def lut_f32(t_u8):
    """The fp32 (B, 1, S, S) tensor holding the values the bytes stand for (CPU)."""
    from signature_gan_amd import _lib
    return torch.from_numpy(_lib.dequant_table())[t_u8.cpu().long()].unsqueeze(1).contiguous()
