"""Shared by the parameter-gradient and adaptation tests (and profiles/param_grad_parity_margins.py): the fp64 oracle side of the
per-image objective  w_r * mean((G(z) - t)^2) + w_d * -log D(G(z))  differentiated with respect to the Generator's PARAMETERS
through the eval-mode Generator (BatchNorm = the affine of its running statistics) and the eval-mode Discriminator, and the
adaptation loop's case."""
import torch
import torch.nn.functional as F

from common import O
from latentcommon import P_LATENT, P_SIZE, oracle_sd64

PARAM_WEIGHTS = [(1.0, 0.0), (0.0, 1.0), (16.0, 1.0)]      # reconstruction alone, realism alone, both at one order of magnitude
BOUND = 1e-4                                              # max|d - ref| <= BOUND * max|ref| per parameter tensor

# the adaptation loop's case: latentcommon.projection_case() with z0 = z* + 0.25 n as FIXED pivots, final-conv gain 32
A_STEPS, A_LR, A_BETAS, A_GAIN = 12, 1e-4, (0.9, 0.999), 32.0


def param_keys(latent, size):
    return O.param_names(O.g_state_specs(latent, size))


def n_blocks(size):
    return len(O.G_CHAIN[size]) - 1


def oracle_param_grads(g_sd64, d_sd64, z, t64, size, latent, signs_g=None, signs_d=None, slope=0.0, rec_g=None, rec_d=None):
    """({key: d sum_b recon_b / d theta}, {key: d sum_b realism_b / d theta}, terms (2, B), logits (B,)) in fp64.  ``signs_*``:
    another implementation's activation decisions (None: the run's own); ``d_sd64`` None: no realism term (zeros).  The
    objective is linear in the two terms, so one run serves every weight pair."""
    keys = param_keys(latent, size)
    sd = {k: (v.clone().requires_grad_() if k in keys else v) for k, v in g_sd64.items()}
    leaves = [sd[k] for k in keys]
    img = O.g_forward(sd, z.double(), False, size, signs=signs_g, record=rec_g, slope=slope)
    recon = ((img[:, 0] - t64) ** 2).mean(dim=(1, 2))
    zero = {k: torch.zeros_like(sd[k]) for k in keys}
    if d_sd64 is not None:
        feat = O.d_features(d_sd64, img, size, None, signs=signs_d, record=rec_d)
        logit = F.linear(feat, d_sd64["classifier.0.weight"], d_sd64["classifier.0.bias"])[:, 0]
        real = F.softplus(-logit)                                        # -log sigmoid(x)
        g_real = dict(zip(keys, torch.autograd.grad(real.sum(), leaves, retain_graph=True)))
    else:
        logit, real, g_real = torch.zeros_like(recon), torch.zeros_like(recon), zero
    g_recon = dict(zip(keys, torch.autograd.grad(recon.sum(), leaves)))
    return g_recon, g_real, torch.stack([recon.detach(), real.detach()]), logit.detach()


def combine(w, g_recon, g_real):
    return {k: float(w[0]) * g_recon[k] + float(w[1]) * g_real[k] for k in g_recon}


def split_arena(eng, flat):
    """{key: CPU copy of the tensor's span of a flat arena-shaped tensor}."""
    flat = flat.detach().cpu()
    return {k: flat[o:o + n].view(shape).clone() for k, (o, n, shape) in eng.g_spans.items()}


def tensor_margins(got, ref):
    """{key: (max|got - ref| / max|ref|, max|ref|)}."""
    return {k: (float((got[k].double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300), float(ref[k].abs().max()))
            for k in ref}


def oracle_adapt(z, t64, first_layer, steps=A_STEPS, lr=A_LR, betas=A_BETAS, gain=A_GAIN):
    """adapt_generator's loop on the CPU (reconstruction only, no anchor): the oracle in fp64 under torch.optim.Adam on the same
    trainable set, the gradient of the MEAN over the N targets.  Returns the (steps, N) loss history (the loss at the start of
    every iteration)."""
    from signature_gan_amd.layout import adaptation_plan
    sd = oracle_sd64(P_SIZE, P_LATENT, gain)
    train = adaptation_plan(first_layer, n_blocks(P_SIZE))[0]
    for k in train:
        sd[k] = sd[k].clone().requires_grad_()
    opt = torch.optim.Adam([sd[k] for k in train], lr=lr, betas=betas)
    hist = []
    for _ in range(steps):
        opt.zero_grad()
        img = O.g_forward(sd, z.double(), False, P_SIZE)
        loss = ((img[:, 0] - t64) ** 2).mean(dim=(1, 2))
        loss.mean().backward()
        hist.append(loss.detach().clone())
        opt.step()
    return torch.stack(hist)
