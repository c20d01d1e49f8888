"""Shared by the latent-gradient and projection tests: the fp64 oracle side of the reconstruction loss mean((G(z) - t)^2)
through the eval-mode Generator, and the projection case both the loop tests and profiles/projection_parity_margins.py run."""
import numpy as np
import torch

from common import I, O, SEED, oracle_states

# the loop tests' case: 64x64, latent 100, three targets; start at z* + 0.25 n (z* generated the targets), Adam lr 0.02, 40 steps
P_SIZE, P_LATENT, P_N, P_STEPS, P_LR, P_BETAS, P_NOISE = 64, 100, 3, 40, 0.02, (0.9, 0.999), 0.25


def oracle_sd64(size, latent, gain=1.0):
    """The synthetic Generator state in fp64 (counters stay integers), the final conv multiplied by ``gain``."""
    sd = oracle_states(size, latent, warm=False)[0]
    sd["final_conv.0.weight"] = sd["final_conv.0.weight"] * gain
    sd["final_conv.0.bias"] = sd["final_conv.0.bias"] * gain
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def oracle_latent_grad(sd64, z, t64, size, signs=None, slope=0.0, record=None):
    """(dz, loss) of the reconstruction loss in fp64 through the oracle's eval-mode Generator; ``signs``: another
    implementation's activation decisions for the backward pass (None: the run's own)."""
    z64 = z.double().clone().requires_grad_()
    img = O.g_forward(sd64, z64, False, size, signs=signs, record=record, slope=slope)
    loss = ((img[:, 0] - t64) ** 2).mean(dim=(1, 2))
    loss.sum().backward()
    return z64.grad.detach(), loss.detach()


def projection_case():
    """(state dict fp32, z* (N, latent), z0 (N, latent)) of the loop tests' case."""
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in I.gen_state(O.g_state_specs(P_LATENT, P_SIZE), SEED["state_g"]).items()}
    z_star = torch.from_numpy(I.gen_z(P_N, P_LATENT, SEED["z"]))
    z0 = z_star + P_NOISE * torch.randn(P_N, P_LATENT, generator=torch.Generator().manual_seed(17))
    return sd, z_star, z0


def oracle_descent(t64, z0):
    """The same loop on the CPU: the oracle in fp64 under torch.optim.Adam.  Returns the (steps, N) loss history (the loss at
    the start of every iteration)."""
    sd64 = oracle_sd64(P_SIZE, P_LATENT)
    z = z0.double().clone().requires_grad_()
    opt = torch.optim.Adam([z], lr=P_LR, betas=P_BETAS)
    hist = []
    for _ in range(P_STEPS):
        opt.zero_grad()
        img = O.g_forward(sd64, z, False, P_SIZE)
        loss = ((img[:, 0] - t64) ** 2).mean(dim=(1, 2))
        loss.sum().backward()
        hist.append(loss.detach().clone())
        opt.step()
    return torch.stack(hist)
