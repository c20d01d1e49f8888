"""The signature verifier's eval-mode forward restated with torch functionals (the yardstick for cases that have no
fixture), the fixtures' loader and the parity bound.

Bound (per tensor): 32 x the reference's own fp32-vs-fp64 deviation stored in the fixture -- relative to the tensor's
max-abs for the stage probes, absolute for embeddings and scores -- and never looser than 1e-4.  The forward pass is
continuous (ReLU and max have no jumps in value), so a different summation order over K <= 8192 moves a result by a small
multiple of the reference's own rounding; 32 covers it."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import inputs as I                                   # noqa: E402
import verifier_inputs as VI                         # noqa: E402

MARGIN, CAP = 32.0, 1e-4
BN_EPS = 1e-5


def torch_state(e=128, seed=VI.SEED["state"], dtype=torch.float32, device="cpu"):
    out = {}
    for k, a in VI.gen_state(e, seed).items():
        t = torch.from_numpy(np.asarray(a))
        out[k] = (t.to(dtype) if t.is_floating_point() else t).to(device)
    return out


def encode(sd, x, taps=None):
    """CNNEncoder.forward in eval mode; taps: dict that receives pool1 / pool2 / pool3 (NCHW) and fc1 (after ReLU)."""
    for i, pad in ((1, 2), (2, 2), (3, 1)):
        p = f"encoder.conv{i}"
        b = f"encoder.bn{i}"
        x = F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=1, padding=pad)
        x = F.batch_norm(x, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"], False, 0.1, BN_EPS)
        x = F.max_pool2d(F.relu(x), 2, 2)
        if taps is not None:
            taps[f"pool{i}"] = x
    x = F.relu(F.linear(x.reshape(x.size(0), -1), sd["encoder.fc1.weight"], sd["encoder.fc1.bias"]))
    if taps is not None:
        taps["fc1"] = x
    x = F.linear(x, sd["encoder.fc2.weight"], sd["encoder.fc2.bias"])
    return F.normalize(x, p=2, dim=1)


def head(sd, e1, e2):
    h = F.relu(F.linear(torch.abs(e1 - e2), sd["classifier.0.weight"], sd["classifier.0.bias"]))
    return torch.sigmoid(F.linear(h, sd["classifier.3.weight"], sd["classifier.3.bias"]))


def forward(sd, x1, x2, taps=None):
    """SiameseNetwork.forward in eval mode: (e1, e2, similarity (B, 1)); taps hold the stages of cat(x1, x2)."""
    with torch.no_grad():
        t1, t2 = ({}, {}) if taps is not None else (None, None)
        e1, e2 = encode(sd, x1, t1), encode(sd, x2, t2)
        if taps is not None:
            for k in t1:
                taps[k] = torch.cat([t1[k], t2[k]], dim=0)
        return e1, e2, head(sd, e1, e2)


def case_inputs(n_pairs):
    """(x1, x2, x2 bytes) of a fixture case as torch CPU tensors."""
    return (torch.from_numpy(VI.gen_x1(n_pairs)), torch.from_numpy(VI.gen_x2(n_pairs)),
            torch.from_numpy(VI.gen_x2_bytes(n_pairs)))


def load_case(n_pairs, e):
    return np.load(os.path.join(GOLDEN, VI.case_name(n_pairs, e) + ".npz"))


def load_manifest():
    with open(os.path.join(GOLDEN, "verifier_manifest.json")) as f:
        return json.load(f)


def probe(t, name):
    a = t.detach().reshape(-1).cpu().numpy()
    return a[I.probe_idx(a.size, "verifier:" + name)]


def bound(f, name):
    """Absolute bound for tensor `name` of fixture f ('e1' | 'e2' | 'similarity' | a stage)."""
    ref64, ref32 = f[name + "_f64"], f[name + "_f32"].astype(np.float64)
    dev = float(np.abs(ref32 - ref64).max())
    if name in ("e1", "e2", "similarity"):
        return min(MARGIN * dev, CAP)
    scale = float(np.abs(ref64).max())
    return min(MARGIN * dev / scale, CAP) * scale


def deviation(got, f, name):
    """max |got - fp64 reference|; got: the full tensor for e1 / e2 / similarity, the probed values for a stage."""
    return float(np.abs(np.asarray(got, np.float64).reshape(-1) - f[name + "_f64"].reshape(-1)).max())


def check(got, f, name, what, margins=None):
    d, b = deviation(got, f, name), bound(f, name)
    print(f"{what} {name}: deviation {d:.3e} bound {b:.3e}")
    if margins is not None:
        margins[name] = {"deviation": d, "bound": b}
    assert d <= b, f"{what} {name}: deviation {d:.3e} exceeds bound {b:.3e}"
