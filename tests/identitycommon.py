"""The verifier's eval-mode INPUT gradient (siggan_verifier_input_grad) restated in fp64 with torch functionals, taking the
pooling routes, the two ReLU masks and the signs of e - r as INPUTS, the way verifiertraincommon.train_grads does for the train
step: the routed window element is gathered and multiplied by `route < 4`, a ReLU is a multiplication by its mask, |u| is
u * sign, and autograd does the rest.  With its own decisions it is torch.autograd on verifiercommon.encode / head
(tests/test_identity_cpu.py pins it); given the HIP path's decisions it is the yardstick the HIP arithmetic is compared with.

The state is verifiercommon's synthetic one with two edge channels in bn2: one gamma < 0 and one gamma == 0 (the un-pool's
scale must be right for both)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import verifiercommon as VC                          # noqa: E402
import verifiertraincommon as TC                     # noqa: E402
from verifiercommon import VI                        # noqa: E402
from verifiertraincommon import TI                   # noqa: E402

BOUND = 1e-4                                         # README parity contract: HIP = oracle(HIP's decisions), relative to max-abs
NEAR_TIE = TI.NEAR_TIE                               # the trainer tests' borderline criterion
GAMMA_NEG, GAMMA_ZERO = 3, 5                         # bn2 channels
ROUTES = {"route1": (32, 32, 32), "route2": (64, 16, 16), "route3": (128, 8, 8)}
DECISIONS = ("route1", "route2", "route3", "fc1_mask", "cls_mask", "diff_sign")
WEIGHTS = ((1.0, 0.0), (0.0, 1.0), (0.5, 2.0))


def identity_state(e=128, dtype=torch.float64, device="cpu"):
    """verifiercommon's state with bn2.weight[GAMMA_NEG] < 0 and bn2.weight[GAMMA_ZERO] == 0."""
    sd = VC.torch_state(e, dtype=dtype, device=device)
    g = sd["encoder.bn2.weight"].clone()
    g[GAMMA_NEG] = -g[GAMMA_NEG].abs()
    g[GAMMA_ZERO] = 0.0
    sd["encoder.bn2.weight"] = g
    return sd


def images(n):
    """(x, targets): the images the gradient is taken at and the images whose embeddings are the references, fp32."""
    return torch.from_numpy(VI.gen_x1(n)), torch.from_numpy(VI.gen_x2(n))


def input_grad_ref(sd, x, r, w_e, w_s, decisions=None, margins=None):
    """fp64 terms and dx of  w_e * 0.5 * sum (e - r)^2 + w_s * -max(log s, -100)  per image.  decisions: None (take them) or
    {"route1|2|3" (N, C, h, w), "fc1_mask" (N, 512), "cls_mask" (N, 64) uint8, "diff_sign" (N, E) int8}.  margins: a dict that
    receives every decision's relative margin (route_margin / mask_margin).  Returns a dict: dx, objective (N), terms (2, N)
    unweighted with 0 where the weight is 0, score (N), logit (N), emb (N, E), decisions."""
    dt = sd["encoder.fc1.weight"].dtype
    x = x.detach().to(dt).clone().requires_grad_(True)
    r = r.detach().to(dt)
    dec = {}
    h = x
    for i, pad in ((1, 2), (2, 2), (3, 1)):
        c, b = f"encoder.conv{i}", f"encoder.bn{i}"
        y = F.conv2d(h, sd[c + ".weight"], sd[c + ".bias"], stride=1, padding=pad)
        z = F.batch_norm(y, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"], False, 0.1, VC.BN_EPS)
        rt = TC.route_of(z) if decisions is None else torch.as_tensor(decisions[f"route{i}"])
        dec[f"route{i}"] = rt
        if margins is not None:
            margins[f"route{i}"] = TC.route_margin(z)
        g = torch.gather(TC.windows(z), -1, rt.clamp(max=3).to(torch.int64).unsqueeze(-1)).squeeze(-1)
        h = g * (rt < 4).to(dt)
    pre = F.linear(h.reshape(h.size(0), -1), sd["encoder.fc1.weight"], sd["encoder.fc1.bias"])
    m = (pre.detach() > 0) if decisions is None else torch.as_tensor(decisions["fc1_mask"]).bool()
    dec["fc1_mask"] = m.to(torch.uint8)
    e = F.normalize(F.linear(pre * m.to(dt), sd["encoder.fc2.weight"], sd["encoder.fc2.bias"]), p=2, dim=1)
    d = e - r
    sg = torch.sign(d.detach()) if decisions is None else torch.as_tensor(decisions["diff_sign"]).to(dt)
    dec["diff_sign"] = sg.to(torch.int8)
    pre_c = F.linear(d * sg, sd["classifier.0.weight"], sd["classifier.0.bias"])
    mc = (pre_c.detach() > 0) if decisions is None else torch.as_tensor(decisions["cls_mask"]).bool()
    dec["cls_mask"] = mc.to(torch.uint8)
    if margins is not None:
        margins["fc1_mask"], margins["cls_mask"] = TC.mask_margin(pre), TC.mask_margin(pre_c)
        margins["diff_sign"] = d.detach().abs() / d.detach().abs().max()
    logit = F.linear(pre_c * mc.to(dt), sd["classifier.3.weight"], sd["classifier.3.bias"]).squeeze(1)
    s = torch.sigmoid(logit)
    zero = torch.zeros_like(logit)
    te = 0.5 * (d * d).sum(dim=1) if w_e > 0 else zero
    ts = -torch.clamp(torch.log(s), min=-100.0) if w_s > 0 else zero
    obj = w_e * te + w_s * ts
    obj.sum().backward()
    return dict(dx=x.grad.detach(), objective=obj.detach(), terms=torch.stack([te.detach(), ts.detach()]), score=s.detach(),
                logit=logit.detach(), emb=e.detach(), decisions=dec)


def autograd_ref(sd, x, r, w_e, w_s):
    """The same objective straight through verifiercommon.encode / head and torch.autograd: (dx, objective)."""
    dt = sd["encoder.fc1.weight"].dtype
    x = x.detach().to(dt).clone().requires_grad_(True)
    r = r.detach().to(dt)
    e = VC.encode(sd, x)
    s = VC.head(sd, e, r).squeeze(1)
    obj = w_e * 0.5 * ((e - r) ** 2).sum(dim=1) + w_s * -torch.clamp(torch.log(s), min=-100.0)
    obj.sum().backward()
    return x.grad.detach(), obj.detach()


def dead_fraction(dec):
    """Per layer: the share of pooled elements whose window maximum is not positive (route 4)."""
    return {k: float((torch.as_tensor(dec[k]) == 4).double().mean()) for k in ROUTES}


def differing(dec_a, dec_b, margins):
    """Per decision: (#positions where the two runs differ, #of those the fp64 run calls borderline: margin < NEAR_TIE)."""
    out = {}
    for k in DECISIONS:
        diff = (torch.as_tensor(dec_a[k]).to(torch.int16) != torch.as_tensor(dec_b[k]).to(torch.int16)).reshape(-1)
        near = (margins[k].reshape(-1) < NEAR_TIE)
        out[k] = (int(diff.sum()), int((diff & near).sum()))
    return out
