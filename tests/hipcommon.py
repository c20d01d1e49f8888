"""Helpers for the GPU parity tests: put the synthetic states of tests/golden/inputs.py into an
Engine (the HIP path) exactly as common.oracle_states() puts them into the oracle."""
import numpy as np
import torch

from common import I, O, SEED

import signature_gan_amd                      # noqa: F401  (import shim for signature-gan_amd/)
from signature_gan_amd.engine import Engine


def load_engine_state(eng, size, latent, warm):
    gs, ds = O.g_state_specs(latent, size), O.d_state_specs(size)
    g_np, d_np = I.gen_state(gs, SEED["state_g"]), I.gen_state(ds, SEED["state_d"])
    gv, dv, bnv = eng.views("g"), eng.views("d"), eng.bn_views()
    for k, a in g_np.items():
        t = torch.from_numpy(np.asarray(a))
        (gv[k] if k in gv else bnv[k]).copy_(t)
    for k, a in d_np.items():
        dv[k].copy_(torch.from_numpy(a))
    for which, specs, seed in (("g", gs, SEED["adam_g"]), ("d", ds, SEED["adam_d"])):
        mv, vv = eng.views(which, "exp_avg"), eng.views(which, "exp_avg_sq")
        steps = getattr(eng, f"{which}_adam_steps")
        if warm:
            m, v, step = I.gen_adam(specs, seed)
            for k in m:
                mv[k].copy_(torch.from_numpy(m[k])); vv[k].copy_(torch.from_numpy(v[k]))
            steps.fill_(float(step))
        else:
            getattr(eng, f"{which}_exp_avg").zero_(); getattr(eng, f"{which}_exp_avg_sq").zero_(); steps.zero_()
    eng.g_grads.zero_(); eng.d_grads.zero_()
    eng.params_changed()
    return eng


def make_engine(size, latent, max_batch, warm=False, seed=0, dtype="f32"):
    eng = Engine(latent_dim=latent, image_size=size, max_batch=max_batch, device="cuda:0", seed=seed, dtype=dtype)
    return load_engine_state(eng, size, latent, warm)


def cuda(a):
    return torch.as_tensor(a).to("cuda:0")


def oracle_state_of(eng, size, latent):
    """The engine's complete training state as oracle dicts (copies on the CPU): g_sd (parameters + BatchNorm buffers), d_sd,
    and both Adam states."""
    gs, ds = O.g_state_specs(latent, size), O.d_state_specs(size)
    cp = lambda d: {k: t.detach().float().cpu().clone() for k, t in d.items()}
    g_par, d_par, bn = cp(eng.views("g")), cp(eng.views("d")), eng.bn_views()
    g_sd = {}
    for k, (_, kind) in gs.items():
        g_sd[k] = g_par[k] if kind == "param" else (bn[k].detach().cpu().clone() if kind == "counter" else bn[k].detach().float().cpu().clone())
    opts = []
    for which, specs, sd in (("g", gs, g_sd), ("d", ds, d_par)):
        o = O.AdamState(O.param_names(specs), sd)
        o.m, o.v = cp(eng.views(which, "exp_avg")), cp(eng.views(which, "exp_avg_sq"))
        o.step = int(float(getattr(eng, f"{which}_adam_steps")[0]))
        opts.append(o)
    return g_sd, d_par, opts[0], opts[1]


# ---- the benchmark's loop (bench.py, --gpus 1) ----------------------------------------------------------------
def bench_setup(dtype, size, latent, batch):
    """Engine, DataParallelStep and real batch exactly as bench.py builds them for one GPU: context seed 2 (library RNG),
    init_reference(seed=0) with fresh Adam state, default execution mode (overlap, no graph), no process group."""
    from signature_gan_amd.dp import DataParallelStep
    eng = Engine(latent_dim=latent, image_size=size, max_batch=batch, device="cuda:0", seed=2, dtype=dtype)
    eng.init_reference(seed=0)
    dp = DataParallelStep(eng, transport="host")
    dp.sync_initial_state()
    gen = torch.Generator(device="cpu").manual_seed(1)
    real = (torch.rand(batch, 1, size, size, generator=gen) * 2 - 1).to("cuda:0")
    return eng, dp, real


def full_state(eng):
    """Copies of everything a step changes: both networks' parameters and Adam moments / step counts, the BatchNorm
    buffers and the 16 metrics."""
    return {n: getattr(eng, n).clone() for n in ("g_params", "d_params", "g_exp_avg", "g_exp_avg_sq", "d_exp_avg", "d_exp_avg_sq",
                                                 "g_adam_steps", "d_adam_steps", "g_bn_mean", "g_bn_var", "g_bn_batches", "metrics")}


def assert_same_state(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


def hip_d_masks(eng, size, batch):
    """The dropout keep masks the last D step used (debug 'd_noise' > 0): D(real) blocks then D(fake) blocks, (B, C_l) each,
    in the order the oracle's d_step takes them."""
    noise = [eng.debug_tensor("d_noise", l, (2 * batch, c)).cpu() for l, c in enumerate(O.D_CHAIN[size], start=1)]
    return [(t[:batch] > 0).float() for t in noise] + [(t[batch:] > 0).float() for t in noise]


def debug_scalar(eng, name):
    return float(eng.debug_tensor(name, 0, (1,)).item())


# ---- sign decisions of the HIP path (borderline activations) -------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def hip_signs_d(eng, size, batch, passes):
    """Sign decisions (activation > 0) the HIP path took in the Discriminator, per pass and
    block, NCHW bool -- handed to the oracle's backward (oracle._ActWithGivenSign).  passes == 1: the Discriminator pass
    of a G step (debug tensor 'd_a_g': wherever the library put those rows); 2: D(real), D(fake) of a D step."""
    out = []
    name = "d_a_g" if passes == 1 else "d_a"
    for p in range(passes):
        for l, c in enumerate(list(O.D_CHAIN[size]), start=1):
            h = size >> l
            a = eng.debug_tensor(name, l, (passes * batch, h, h, c))[p * batch:(p + 1) * batch]
            out.append(_nchw(a) > 0)
    return out


def hip_signs_g(eng, size, batch):
    chain = O.G_CHAIN[size]
    out = []
    for l, c in enumerate(chain):
        h = 4 << l
        a = _nchw(eng.debug_tensor("g_a", l, (batch, h, h, c)))
        out.append((a > 0).reshape(batch, -1) if l == 0 else a > 0)
    return out


def hip_ablation_iteration(eng, real, z, masks, size, batch):
    """One iteration of the 'ablation' step variant phase by phase (what Engine.ablation_step does), reading the sign decisions
    where they still stand.  ``masks``: the three passes' dropout masks.  Returns (metrics, signs, keep, d_grads, g_grads,
    probs): ``signs`` in the named groups oracle.ablation_step takes, ``keep`` the dropout masks of the same groups (for
    count_sign_flips), the two gradient arenas as CPU copies, and the per-sample Discriminator outputs of the three passes,
    (3, batch)."""
    nb = len(masks) // 3
    eng.d_compute_grads(cuda(real), cuda(z), masks, 0.9, mask_passes=3)
    s_g, s_d = hip_signs_g(eng, size, batch), hip_signs_d(eng, size, batch, 2)
    d_grads = {k: v.cpu().clone() for k, v in eng.views("d", "grads").items()}
    probs = [eng.debug_tensor("probs", 0, (2 * batch,)).cpu().clone()]
    met = eng.d_apply()
    eng.g_compute_grads(batch, label_smoothing=0.9)
    s_dg = hip_signs_d(eng, size, batch, 1)
    probs.append(eng.debug_tensor("probs", 0, (batch,)).cpu().clone())
    met.update(eng.g_apply())
    g_grads = {k: v.cpu().clone() for k, v in eng.views("g", "grads").items()}
    signs = {"g": s_g, "d_real": s_d[:nb], "d_fake": s_d[nb:], "d_g": s_dg}
    keep = {"g": None, "d_real": masks[:nb], "d_fake": masks[nb:2 * nb], "d_g": masks[2 * nb:]}
    return met, signs, keep, d_grads, g_grads, torch.cat(probs).reshape(3, batch)


def grad_scales(o_grads, names):
    """Per-tensor comparison scale of a gradient arena against an oracle's: the tensor's largest gradient, floored at 1e-3 of
    the network's (1e-2 for the Linear bias in front of BatchNorm1d, whose true gradient is zero)."""
    gscale = max(float(o_grads[k].abs().max()) for k in names)
    return {k: max(float(o_grads[k].abs().max()), (1e-2 if k == "fc.0.bias" else 1e-3) * gscale) for k in names}


def count_sign_flips(signs, recorded, keep=None):
    """Disagreements between the HIP sign decisions and the oracle's own; every one must be a
    pre-activation within rounding of zero (|x| <= 1e-5 of the layer's scale).  Their NUMBER is bounded too, in proportion to
    the activations compared: two fp32 implementations differ by ~1e-7 of a layer's scale, so of N inputs spread over that
    scale about 1e-7 N (times the density at zero) land on the other side -- 16, or one per million where that is more (the
    128x128 batch-32 steps compare 41 M activations; 12-17 were seen there across boxes, whose oracle runs with different
    thread counts)."""
    n, total = 0, 0
    for i, (s, x) in enumerate(zip(signs, recorded)):
        total += x.numel()
        bad = s.reshape(x.shape) != (x > 0)
        if keep is not None and keep[i] is not None:
            bad &= keep[i][:, :, None, None] > 0          # dropped planes carry no gradient
        if bad.any():
            assert float(x[bad].abs().max()) <= 1e-5 * float(x.abs().max()), "sign disagreement away from zero"
            n += int(bad.sum())
    assert n <= max(16, total // 1000000), f"{n} borderline sign decisions differ (of {total} activations)"
    return n
