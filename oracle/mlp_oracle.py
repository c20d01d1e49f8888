"""CPU restatement of the fully-connected GAN extension.  TEST INFRASTRUCTURE ONLY (see oracle/siggan_oracle.py's header).

PARITY UNPINNED: the reference contains no fully-connected Generator / Discriminator (generator_vanilla_gan.py:106-107 and
discriminator_vanilla_gan.py:121-122 reject everything but the 64 / 128 conv models; no test, fixture or golden vector of
the reference covers an MLP), so this file is the build's own definition of BASELINE.json's configs[0] model, restated with
torch-CPU functional ops -- it checks that the HIP path computes what include/siggan_mlp.h says, not that it matches the
reference.  The step structure, loss, label smoothing and Adam follow the reference's conv path
(vanilla_gan_model.py:180-306, restated in siggan_oracle.py), from which bce / adam_update are reused."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from .siggan_oracle import AdamState, BN_EPS, BN_MOMENTUM, bce, clip_grad_norm

Tensor = torch.Tensor


def g_forward(sd: Dict[str, Tensor], z: Tensor, hidden, size: int, training: bool, taps: Optional[dict] = None) -> Tensor:
    """taps (optional dict) receives, per hidden layer, the Linear output ("g_lin", attached to the graph) and the BatchNorm
    output the ReLU decides on ("g_post_bn", detached)."""
    x = z
    for i in range(len(hidden)):
        x = F.linear(x, sd[f"net.{i}.linear.weight"], sd[f"net.{i}.linear.bias"])
        if taps is not None:
            taps.setdefault("g_lin", []).append(x)
        if training:
            sd[f"net.{i}.bn.num_batches_tracked"] += 1
        x = F.batch_norm(x, sd[f"net.{i}.bn.running_mean"], sd[f"net.{i}.bn.running_var"], sd[f"net.{i}.bn.weight"],
                         sd[f"net.{i}.bn.bias"], training, BN_MOMENTUM, BN_EPS)
        if taps is not None:
            taps.setdefault("g_post_bn", []).append(x.detach())
        x = F.relu(x)
    x = torch.tanh(F.linear(x, sd["out.weight"], sd["out.bias"]))
    return x.view(-1, 1, size, size)


def d_forward(sd: Dict[str, Tensor], x: Tensor, n_hidden: int, slope: float = 0.2, taps: Optional[dict] = None) -> Tensor:
    """taps (optional dict) receives, per hidden layer, the value the LeakyReLU decides on ("d_pre", detached)."""
    x = x.flatten(1)
    for j in range(n_hidden):
        x = F.linear(x, sd[f"net.{j}.weight"], sd[f"net.{j}.bias"])
        if taps is not None:
            taps.setdefault("d_pre", []).append(x.detach())
        x = F.leaky_relu(x, slope)
    return torch.sigmoid(F.linear(x, sd["out.weight"], sd["out.bias"]))


def _leafs(sd, names):
    return {k: sd[k].detach().clone().requires_grad_(True) for k in names}


def d_step(g_sd, d_sd, d_opt: AdamState, real, z, hidden, size, lr=2e-4, beta1=0.5, beta2=0.999, label_smoothing=0.9,
           clip: Optional[float] = None, aux: Optional[dict] = None):
    """One Discriminator step, in the dtype of the state it is given.  clip: nn.utils.clip_grad_norm_'s max_norm (the returned
    gradients are then the clipped ones).  aux (optional dict) receives "d_pre": the pre-LeakyReLU values of the real rows then
    of the fake rows, per hidden layer -- the decisions this step's gradients depend on (the eval-mode Generator in front is
    under no_grad: its ReLUs are continuous in value and nothing is differentiated through them) -- and "grad_norm": the
    pre-clip norm (None without clip)."""
    names = d_opt.names
    leaf = _leafs(d_sd, names)
    with torch.no_grad():
        fake = g_forward(g_sd, z, hidden, size, training=False)
    tr, tf = ({}, {}) if aux is not None else (None, None)
    rp, fp = d_forward(leaf, real, len(hidden), taps=tr), d_forward(leaf, fake, len(hidden), taps=tf)
    lr_, lf_ = bce(rp, label_smoothing), bce(fp, 0.0)
    loss = lr_ + lf_
    gl = torch.autograd.grad(loss, [leaf[k] for k in names])
    grads = {k: g.detach() for k, g in zip(names, gl)}
    norm = clip_grad_norm(list(grads.values()), clip) if clip is not None else None
    if aux is not None:
        aux["d_pre"] = [torch.cat([a, b], dim=0) for a, b in zip(tr["d_pre"], tf["d_pre"])]
        aux["grad_norm"] = norm
    d_opt.apply(d_sd, grads, lr, beta1, beta2)
    return {"d_loss": float(loss.detach()), "d_loss_real": float(lr_.detach()), "d_loss_fake": float(lf_.detach()),
            "d_real_mean": float(rp.detach().mean()), "d_fake_mean": float(fp.detach().mean())}, grads


def g_step(g_sd, d_sd, g_opt: AdamState, z, hidden, size, lr=2e-4, beta1=0.5, beta2=0.999, clip: Optional[float] = None,
           aux: Optional[dict] = None):
    """One Generator step, in the dtype of the state it is given; clip as in d_step.  aux (optional dict) receives
    "g_post_bn" and "d_pre" (the values the Generator's ReLUs and the Discriminator's LeakyReLUs decide on, per hidden layer),
    "grad_norm" (the pre-clip norm, None without clip) and "lin_bias_terms": per hidden layer the largest column sum of
    |dL/dy| over the Linear outputs y.  The gradient of a Linear bias in front of a train-mode BatchNorm is that column's
    signed sum, which is zero in exact arithmetic: what any implementation holds for it is the rounding of those terms."""
    names = g_opt.names
    leaf = dict(g_sd)
    leaf.update(_leafs(g_sd, names))
    tg, td = ({}, {}) if aux is not None else (None, None)
    fake = g_forward(leaf, z, hidden, size, training=True, taps=tg)
    for k in g_sd:
        if k not in names:
            g_sd[k] = leaf[k]
    fp = d_forward(d_sd, fake, len(hidden), taps=td)
    loss = bce(fp, 1.0)
    lin = tg["g_lin"] if aux is not None else []
    gl = torch.autograd.grad(loss, [leaf[k] for k in names] + lin)
    grads = {k: g.detach() for k, g in zip(names, gl)}
    norm = clip_grad_norm(list(grads.values()), clip) if clip is not None else None
    if aux is not None:
        aux["g_post_bn"], aux["d_pre"], aux["grad_norm"] = tg["g_post_bn"], td["d_pre"], norm
        coef = min(1.0, clip / (norm + 1e-6)) if clip is not None else 1.0         # (the clipped gradients' terms are scaled alike)
        aux["lin_bias_terms"] = [coef * float(g.detach().abs().sum(0).max()) for g in gl[len(names):]]
    g_opt.apply(g_sd, grads, lr, beta1, beta2)
    return {"g_loss": float(loss.detach()), "g_fake_mean": float(fp.detach().mean())}, grads
