"""Throughput of the HIP verifier train step (siggan_verifier_train_step) on the MI355X, next to PyTorch-ROCm eager on the
same card.

    python profiles/verifier_train_throughput.py --out profiles/verifier_train_throughput.json

Times one fused train step (forward, BCE + contrastive loss, backward, Adam; dropout masks drawn by the library) at 32 and
128 pairs with HIP events: warm-up, then REPEATS windows of ITERS steps each; the median window and the spread (min / max)
are reported.  In the same process, alternating with the HIP windows, the same step runs in PyTorch-ROCm eager: the
functional network of tests/verifiertraincommon.py with F.relu / F.max_pool2d / F.dropout in place of the forced decisions,
autograd and torch.optim.Adam -- what a user of the reference runs today.  Reported, not gated: the parent has no verifier
training to compare with.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np                                                    # noqa: E402
import torch                                                          # noqa: E402
import torch.nn.functional as F                                       # noqa: E402

import verifiertraincommon as TC                                      # noqa: E402
from verifiertraincommon import TI, VI                                # noqa: E402
from test_verifier_train_gpu import DEV, Rig                          # noqa: E402
from signature_gan_amd import _lib                                    # noqa: E402
from signature_gan_amd.signature_verifier_eval import _ptr            # noqa: E402

REPEATS, ITERS, WARMUP = 7, 10, 3
# per image: conv2 32x32x64 outputs x K = 800, conv3 16x16x128 x K = 576; forward + input gradient + weight gradient
CONV_FLOP = 2 * (32 * 32 * 64 * 800 + 16 * 16 * 128 * 576)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def stats(ts, pairs):
    ts = np.asarray(ts)
    return {"ms_per_step_median": float(np.median(ts) * 1e3), "ms_per_step_min": float(ts.min() * 1e3),
            "ms_per_step_max": float(ts.max() * 1e3), "pairs_per_second_median": float(pairs / np.median(ts))}


def eager_step(P, R, opt, x1, x2, y):
    """The reference's train_epoch body with torch functionals, train mode."""
    def enc(x):
        for i, pad in ((1, 2), (2, 2), (3, 1)):
            c, b = f"encoder.conv{i}", f"encoder.bn{i}"
            x = F.conv2d(x, P[c + ".weight"], P[c + ".bias"], padding=pad)
            x = F.batch_norm(x, R[b + ".running_mean"], R[b + ".running_var"], P[b + ".weight"], P[b + ".bias"], True, 0.1, TC.BN_EPS)
            x = F.max_pool2d(F.relu(x), 2, 2)
        x = F.dropout(F.relu(F.linear(x.reshape(x.size(0), -1), P["encoder.fc1.weight"], P["encoder.fc1.bias"])), 0.5, True)
        return F.normalize(F.linear(x, P["encoder.fc2.weight"], P["encoder.fc2.bias"]), p=2, dim=1)
    opt.zero_grad()
    e1, e2 = enc(x1), enc(x2)
    h = F.dropout(F.relu(F.linear(torch.abs(e1 - e2), P["classifier.0.weight"], P["classifier.0.bias"])), 0.3, True)
    sim = torch.sigmoid(F.linear(h, P["classifier.3.weight"], P["classifier.3.bias"]))
    d = F.pairwise_distance(e1, e2)
    loss = F.binary_cross_entropy(sim.squeeze(1), y) + 0.5 * (y * d.pow(2) + (1 - y) * torch.clamp(2.0 - d, min=0.0).pow(2)).mean()
    loss.backward()
    opt.step()


def measure(pairs):
    rig = Rig(128, pairs)
    rig.t.seed(1, 0)
    x1 = torch.from_numpy(VI.gen_x2(pairs, seed=1)).to(DEV).contiguous()
    x2 = torch.from_numpy(VI.gen_x2(pairs, seed=2)).to(DEV).contiguous()
    y = torch.from_numpy(TI.labels(pairs)).to(DEV)
    metrics = torch.zeros(4, device=DEV)
    lib, h = rig.t.lib, rig.t._h

    def hip():
        _lib.check(lib.siggan_verifier_train_step(h, _ptr(x1), _ptr(x2), _lib.VFMT_F32, _ptr(y), pairs, None, None, 1, TI.LR,
                                                  TI.BETAS[0], TI.BETAS[1], TI.EPS, _ptr(metrics), rig.t.stream()))

    P, R = TC.state(128, torch.float32)
    P = {k: v.to(DEV).requires_grad_(True) for k, v in P.items()}
    R = {k: v.to(DEV) for k, v in R.items()}
    opt = torch.optim.Adam(list(P.values()), lr=TI.LR)
    fns = {"hip": hip, "torch_eager": lambda: eager_step(P, R, opt, x1, x2, y)}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            ts[k].append(window(fn, ITERS))
    out = {k: stats(v, pairs) for k, v in ts.items()}
    out["hip_speedup_over_torch_eager"] = out["torch_eager"]["ms_per_step_median"] / out["hip"]["ms_per_step_median"]
    out["hip"]["conv2_conv3_fwd_dgrad_wgrad_tflops_over_whole_step_time"] = \
        3 * 2 * pairs * CONV_FLOP / (out["hip"]["ms_per_step_median"] * 1e-3) / 1e12
    out["hip"]["last_metrics_loss_bce_contrastive_ncorrect"] = metrics.cpu().tolist()
    rig.t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_train_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    out = {"device": torch.cuda.get_device_name(0), "embedding_dim": 128,
           "method": f"HIP events, {WARMUP} warm-up steps, {REPEATS} windows of {ITERS} steps per path, paths alternated; median and min / max of the windows",
           "pairs": {}}
    for pairs in (32, 128):
        out["pairs"][str(pairs)] = measure(pairs)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
