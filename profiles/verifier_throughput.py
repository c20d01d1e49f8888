"""Throughput of the HIP signature verifier's `score` call on the MI355X, next to PyTorch-ROCm eager on the same card.

    python profiles/verifier_throughput.py --out profiles/verifier_throughput.json [--kernel-stats <rocprofv3 kernel_stats.csv>]

Times siggan_verifier_score (fp32 input and uint8 input) for 32 and 256 pairs with HIP events: warm-up, then REPEATS
windows of ITERS calls each; the median window and the spread (min / max) are reported.  In the same process, alternating
with the HIP windows, the torch restatement of the eval forward (tests/verifiercommon.py) runs under torch.no_grad() in
eager mode -- the path a user of the reference has today.  Reported, not gated.

The share of the fp32 MFMA peak (157.3 TFLOP/s) is given two ways and named for what it is: conv2 + conv3 FLOPs over the
WHOLE call's time (an end-to-end rate, always available), and over the two kernels' own time when a rocprofv3
--kernel-trace --stats csv of a separate run (`--profile-run`: one shape, no timing) is passed with --kernel-stats.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import numpy as np                                                    # noqa: E402
import torch                                                          # noqa: E402

import verifiercommon as VC                                           # noqa: E402
from verifiercommon import VI                                         # noqa: E402
from test_verifier_gpu import DEV, cuda, make_ctx                     # noqa: E402

PEAK_F32_MFMA = 157.3e12
LAUNCHES_PER_SCORE = 6            # k_vconv1, k_vconv (conv2), k_vconv (conv3), k_vfc1, k_vtail, k_vhead
CONV2_FLOP = 2 * 64 * 64 // 4 * 64 * 25 * 32          # per image: 32x32 outputs x 64 channels x K = 800
CONV3_FLOP = 2 * 16 * 16 * 128 * 9 * 64
REPEATS, ITERS, WARMUP = 7, 20, 5


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters           # seconds per call


def stats(ts, pairs):
    ts = np.asarray(ts)
    return {"seconds_per_call_median": float(np.median(ts)), "seconds_per_call_min": float(ts.min()),
            "seconds_per_call_max": float(ts.max()), "pairs_per_second_median": float(pairs / np.median(ts)),
            "pairs_per_second_min": float(pairs / ts.max()), "pairs_per_second_max": float(pairs / ts.min())}


def measure(pairs):
    ctx = make_ctx(128, 2 * pairs)
    sd = VC.torch_state(128, device=DEV)
    b1 = cuda(torch.from_numpy(VI.gen_x2_bytes(pairs, seed=1)))
    b2 = cuda(torch.from_numpy(VI.gen_x2_bytes(pairs, seed=2)))
    x1 = cuda(torch.from_numpy(VI.normalize_bytes(b1.cpu().numpy()))[:, None].contiguous())
    x2 = cuda(torch.from_numpy(VI.normalize_bytes(b2.cpu().numpy()))[:, None].contiguous())
    fns = {"hip_f32": lambda: ctx.score(x1, x2), "hip_u8": lambda: ctx.score(b1, b2),
           "torch_eager_f32": lambda: VC.forward(sd, x1, x2)}
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(REPEATS):                          # alternate the three within every repeat
        for k, fn in fns.items():
            ts[k].append(window(fn, ITERS))
    out = {k: stats(v, pairs) for k, v in ts.items()}
    flop = 2 * pairs * (CONV2_FLOP + CONV3_FLOP)
    for k in ("hip_f32", "hip_u8"):
        out[k]["conv2_conv3_flop_over_whole_call_time_share_of_f32_mfma_peak"] = flop / out[k]["seconds_per_call_median"] / PEAK_F32_MFMA
    out["hip_f32_speedup_over_torch_eager"] = out["torch_eager_f32"]["seconds_per_call_median"] / out["hip_f32"]["seconds_per_call_median"]
    got, ref = ctx.score(x1, x2)[2], VC.forward(sd, x1, x2)[2]
    out["max_abs_score_difference_hip_vs_torch_eager"] = float((got - ref).abs().max())
    ctx.close()
    return out


def kernel_shares(path, pairs, calls):
    """Per-kernel average times of a --profile-run (rocprofv3 --kernel-trace --stats) and the conv kernels' share of peak."""
    out = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "k_v" not in name:
            continue
        short = name[name.index("k_v"):].split("(")[0]
        out[short] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3}
    conv = {k: v for k, v in out.items() if k.startswith("k_vconv<")}
    t = sum(v["average_us"] for v in conv.values()) * 1e-6
    if t > 0:
        out["conv2_conv3_kernel_time_share_of_f32_mfma_peak"] = 2 * pairs * (CONV2_FLOP + CONV3_FLOP) / t / PEAK_F32_MFMA
    out["pairs"] = pairs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_throughput.json"))
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--profile-run", type=int, default=0, metavar="PAIRS", help="only run 20 fp32 score calls of PAIRS pairs (for rocprofv3)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if a.profile_run:
        ctx = make_ctx(128, 2 * a.profile_run)
        x = cuda(torch.from_numpy(VI.gen_x2(a.profile_run)))
        for _ in range(20):
            ctx.score(x, x)
        torch.cuda.synchronize()
        ctx.close()
        return
    out = {"device": torch.cuda.get_device_name(0), "launches_per_score_call": LAUNCHES_PER_SCORE, "embedding_dim": 128,
           "method": f"HIP events, {WARMUP} warm-up calls, {REPEATS} windows of {ITERS} calls per path, paths alternated; median and min / max of the windows",
           "f32_mfma_peak_flops": PEAK_F32_MFMA, "pairs": {}}
    for pairs in (32, 256):
        out["pairs"][str(pairs)] = measure(pairs)
    if a.kernel_stats:
        out["kernels_profiled_run"] = kernel_shares(a.kernel_stats, 256, 20)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
