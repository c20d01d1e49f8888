"""The signature verifier's TRAIN step restated with torch functionals, taking the pooling routes and ReLU masks as
INPUTS: the routed window element is gathered and multiplied by `route < 4`, a ReLU is a multiplication by its mask, and
autograd does the rest.  Given the reference's own decisions this reproduces the reference's fp64 gradients exactly
(tests/test_verifier_train_cpu.py pins it); given the HIP path's decisions it is the yardstick the HIP arithmetic is compared
with -- a pre-activation within rounding of a tie may fall on either side in two fp32 implementations and then moves whole
gradient sums, so decisions and arithmetic are checked separately (README.md, parity contract).

Bound (per tensor, relative to its max-abs): verifiercommon's rule -- 32 x the reference's own fp32-vs-fp64 deviation, never
looser than 1e-4."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import verifier_inputs as VI                         # noqa: E402
import verifier_train_inputs as TI                   # noqa: E402
import verifiercommon as VC                          # noqa: E402

MARGIN, CAP = VC.MARGIN, VC.CAP
BN_EPS = VC.BN_EPS
CONV_BIAS = tuple(f"encoder.conv{i}.bias" for i in (1, 2, 3))
METRICS = ("loss", "bce", "contrastive", "n_correct")


def windows(z):
    """(N, C, H, W) -> (N, C, H/2, W/2, 4): the 2x2 windows, last axis in (dy, dx) row-major order."""
    n, c, h, w = z.shape
    return z.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)


def route_of(z):
    """uint8 (N, C, H/2, W/2): index of the FIRST maximal element of every window, 4 where that maximum is not positive."""
    w = windows(z.detach())
    best, idx = w[..., 0], torch.zeros(w.shape[:-1], dtype=torch.int64)
    for e in (1, 2, 3):
        gt = w[..., e] > best
        best, idx = torch.where(gt, w[..., e], best), torch.where(gt, torch.full_like(idx, e), idx)
    return torch.where(best > 0, idx, torch.full_like(idx, 4)).to(torch.uint8)


def route_margin(z):
    """Relative margin of every routing decision: the winner's distance to the runner-up or to zero, over the layer's
    max-abs."""
    w = windows(z.detach())
    top = torch.topk(w, 2, dim=-1).values
    m = torch.minimum(top[..., 0] - top[..., 1], top[..., 0].abs())
    return m / z.detach().abs().max()


def mask_margin(pre):
    return pre.detach().abs() / pre.detach().abs().max()


def state(e=128, dtype=torch.float64, seed=VI.SEED["state"]):
    """(params in named_parameters() order, running tensors) of verifier_inputs' state."""
    sd = VC.torch_state(e, seed, dtype)
    return (OrderedDict((k, sd[k].clone()) for k in TI.param_names(e)), OrderedDict((k, sd[k].clone()) for k in TI.running_names()))


def zero_moments(params):
    return (OrderedDict((k, torch.zeros_like(v)) for k, v in params.items()),
            OrderedDict((k, torch.zeros_like(v)) for k, v in params.items()))


def case_batch(n_pairs, dtype=torch.float64, step=0):
    x1, x2, _ = VC.case_inputs(n_pairs)
    return dict(x1=x1.to(dtype), x2=x2.to(dtype), labels=torch.from_numpy(TI.labels(n_pairs)).to(dtype),
                fc_keep=torch.from_numpy(TI.fc_keep(n_pairs, step)).to(dtype),
                cls_keep=torch.from_numpy(TI.cls_keep(n_pairs, step)).to(dtype))


def _encode(P, R, x, keep, dec, out_dec, margins):
    """CNNEncoder.forward in train mode on one half; R's running tensors are updated in place.  dec: None (take the
    decisions) or this half's {"route1".., "fc1_mask"}."""
    for i, pad in ((1, 2), (2, 2), (3, 1)):
        c, b = f"encoder.conv{i}", f"encoder.bn{i}"
        y = F.conv2d(x, P[c + ".weight"], P[c + ".bias"], stride=1, padding=pad)
        z = F.batch_norm(y, R[b + ".running_mean"], R[b + ".running_var"], P[b + ".weight"], P[b + ".bias"], True, 0.1, BN_EPS)
        r = route_of(z) if dec is None else dec[f"route{i}"]
        out_dec[f"route{i}"].append(r)
        if margins is not None:
            margins[f"route{i}"].append(route_margin(z))
        g = torch.gather(windows(z), -1, r.clamp(max=3).to(torch.int64).unsqueeze(-1)).squeeze(-1)
        x = g * (r < 4).to(z.dtype)
    pre = F.linear(x.reshape(x.size(0), -1), P["encoder.fc1.weight"], P["encoder.fc1.bias"])
    m = (pre.detach() > 0) if dec is None else dec["fc1_mask"].bool()
    out_dec["fc1_mask"].append(m.to(torch.uint8))
    if margins is not None:
        margins["fc1_mask"].append(mask_margin(pre))
    h = pre * m.to(pre.dtype) * (keep / (1.0 - TI.P_FC))
    return F.normalize(F.linear(h, P["encoder.fc2.weight"], P["encoder.fc2.bias"]), p=2, dim=1)


def train_grads(P, R, batch, use_contrastive=True, decisions=None, margins=None):
    """One forward + backward.  P: parameters (leaf tensors are made here), R: running tensors (updated in place, x1 then
    x2).  decisions: None or {"route1", "route2", "route3" (2B, C, h, w), "fc1_mask" (2B, 512), "cls_mask" (B, 64)} uint8.
    Returns a dict: loss, bce, contrastive, n_correct, e1, e2, similarity (B), distance (B), grads (by name), decisions."""
    B = batch["x1"].shape[0]
    P = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in P.items())
    out_dec = {k: [] for k in TI.DECISIONS}
    mg = {k: [] for k in TI.DECISIONS} if margins is not None else None
    es = []
    for h, x in enumerate((batch["x1"], batch["x2"])):
        dec = None if decisions is None else {k: torch.as_tensor(decisions[k])[h * B:(h + 1) * B] for k in TI.DECISIONS[:4]}
        es.append(_encode(P, R, x, batch["fc_keep"][h * B:(h + 1) * B], dec, out_dec, mg))
    e1, e2 = es
    pre = F.linear(torch.abs(e1 - e2), P["classifier.0.weight"], P["classifier.0.bias"])
    m = (pre.detach() > 0) if decisions is None else torch.as_tensor(decisions["cls_mask"]).bool()
    out_dec["cls_mask"].append(m.to(torch.uint8))
    if mg is not None:
        mg["cls_mask"].append(mask_margin(pre))
    hid = pre * m.to(pre.dtype) * (batch["cls_keep"] / (1.0 - TI.P_CLS))
    sim = torch.sigmoid(F.linear(hid, P["classifier.3.weight"], P["classifier.3.bias"]))
    y = batch["labels"]
    bce = F.binary_cross_entropy(sim.squeeze(1), y)
    dist = F.pairwise_distance(e1, e2)
    con = (y * dist.pow(2) + (1 - y) * torch.clamp(2.0 - dist, min=0.0).pow(2)).mean()
    loss = bce + 0.5 * con if use_contrastive else bce
    loss.backward()
    if margins is not None:
        margins.update({k: torch.cat(v, dim=0) for k, v in mg.items()})
    pred = (sim.detach().squeeze(1) > 0.5).to(y.dtype)
    return dict(loss=loss.detach(), bce=bce.detach(), contrastive=con.detach() if use_contrastive else torch.zeros_like(con.detach()),
                n_correct=(pred == y).sum().to(y.dtype), e1=e1.detach(), e2=e2.detach(), similarity=sim.detach().squeeze(1),
                distance=dist.detach(), grads=OrderedDict((k, v.grad) for k, v in P.items()),
                decisions={k: torch.cat(v, dim=0) for k, v in out_dec.items()})


def adam_apply(P, grads, m, v, t, lr=TI.LR, betas=TI.BETAS, eps=TI.EPS):
    """torch.optim.Adam's update number t (1-based) in place on P, m, v.  The conv biases are left alone, as the library
    leaves them: their gradient is mathematically zero (a train-mode BatchNorm follows), what autograd holds for them is
    rounding noise that Adam would normalise into a +-lr * |g| / (|g| + eps) walk no output depends on."""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    for k in P:
        if k in CONV_BIAS:
            continue
        g = grads[k]
        m[k].lerp_(g, 1.0 - b1)
        v[k].mul_(b2).addcmul_(g, g, value=1.0 - b2)
        P[k].addcdiv_(m[k], v[k].sqrt() / (bc2 ** 0.5) + eps, value=-lr / bc1)


def load_case(n_pairs, e):
    return np.load(os.path.join(GOLDEN, TI.case_name(n_pairs, e) + ".npz"))


def fixture_decisions(f, prefix):
    return {k: torch.from_numpy(f[f"{prefix}{k}"]) for k in TI.DECISIONS}


def rel_bound(f, key):
    """The bound of tensor `key` (fixture keys key_f32 / key_f64), relative to the fp64 tensor's max-abs."""
    ref64, ref32 = f[key + "_f64"], f[key + "_f32"].astype(np.float64)
    scale = float(np.abs(ref64).max())
    if scale == 0.0:
        return 0.0, 0.0
    return min(MARGIN * float(np.abs(ref32 - ref64).max()) / scale, CAP), scale


def check(got, want, f, key, what, margins=None):
    """got, want: the same positions of a tensor (HIP, fp64 yardstick); the bound comes from fixture f's own fp32 run."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    b, _ = rel_bound(f, key)
    scale = float(np.abs(want).max())
    d = float(np.abs(got - want).max()) / scale if scale > 0 else float(np.abs(got).max())
    print(f"{what} {key}: relative deviation {d:.3e} bound {b:.3e}")
    if margins is not None:
        margins[f"{what} {key}"] = {"deviation": d, "bound": b}
    assert d <= b, f"{what} {key}: relative deviation {d:.3e} exceeds bound {b:.3e}"
