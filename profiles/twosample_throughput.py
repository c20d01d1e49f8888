#!/usr/bin/env python3
"""Time of siggan_kernel_forms on the MI355X against the obvious alternative on the same device and on the host.

    python profiles/twosample_throughput.py [--out profiles/twosample_throughput.json]

Shapes (N rows, P label columns, dim): (1024, 256, 128), (4096, 1024, 128), (4096, 1024, 40); standard-normal fp32 rows
scaled to unit norm, labels uniform over {0, 1, 2}, both already on the device; the RBF kernel (gamma = 1) and the cubic
polynomial one (gamma = 1 / dim, coef0 = 1).  Per shape and kernel:
  "kernel"      utils.twosample.kernel_forms: two launches (three for RBF), a workspace of 24 * ceil(N / 32) * P + 8 N bytes
  "torch_fp64"  the rows widened to fp64, K formed as an (N, N) fp64 matrix from x @ x.T (RBF: norms from its diagonal, d2
                clamped at 0, exp), the diagonal zeroed, Z = K @ [A | B] with the (N, 2 P) fp64 one-hot operand, and the
                element-wise products and column sums -- what one would write with torch ops
  "numpy_host"  the same formulas in numpy on the host, on the threads the machine grants (the environment's OMP_NUM_THREADS
                is recorded), from rows and labels already on the host
WARMUP calls, then ROUNDS samples per device route, the routes alternating; a sample is device events around CALLS back-to-back
calls divided by their number.  The host route: HOST_ROUNDS wall-clock samples of one call.  Medians with min and max.  Also
written: the MFMA flops the kernel issues (K tiles once per 256-column chunk, the RBF norms once per call, and the Z product
over both groups) and that rate as a fraction of the fp64 matrix peak; the useful flops (2 N^2 dim + 2 N^2 2 P) at the kernel's time;
the peak bytes the torch route allocates beyond its inputs against the kernel's workspace; the largest relative difference
between the two device routes.  There is no pass / fail threshold.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import _lib  # noqa: E402
from signature_gan_amd.utils.twosample import kernel_forms  # noqa: E402

WARMUP, ROUNDS, HOST_ROUNDS = 3, 9, 3
SHAPES = [(1024, 256, 128), (4096, 1024, 128), (4096, 1024, 40)]
FP64_MFMA_PEAK_TFLOPS = 78.6                                 # MI355X, matrix fp64 (AMD's product brief)


def torch_route(x, labels, kind, gamma):
    x64 = x.double()
    k = x64 @ x64.T
    if kind == "rbf":
        nrm = torch.diagonal(k).clone()
        k = torch.exp(-gamma * (nrm[:, None] + nrm[None, :] - 2.0 * k).clamp_min_(0.0))
    else:
        t = gamma * k + 1.0
        k = t * t * t
    k.fill_diagonal_(0.0)
    a, b = (labels == 1).double(), (labels == 2).double()
    z = k @ torch.cat([a, b], dim=1)
    p = labels.shape[1]
    return torch.stack([(a * z[:, :p]).sum(0), (b * z[:, p:]).sum(0), (a * z[:, p:]).sum(0)], dim=1)


def numpy_route(x, labels, kind, gamma):
    x64 = x.astype(np.float64)
    k = x64 @ x64.T
    if kind == "rbf":
        nrm = np.diagonal(k).copy()
        k = np.exp(-gamma * np.maximum(nrm[:, None] + nrm[None, :] - 2.0 * k, 0.0))
    else:
        t = gamma * k + 1.0
        k = t * t * t
    np.fill_diagonal(k, 0.0)
    a, b = (labels == 1).astype(np.float64), (labels == 2).astype(np.float64)
    z = k @ np.concatenate([a, b], axis=1)
    p = labels.shape[1]
    return np.stack([(a * z[:, :p]).sum(0), (b * z[:, p:]).sum(0), (a * z[:, p:]).sum(0)], axis=1)


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)}


def issued_mfma_flops(n, p, dim, kind):
    """What csrc/twosample.hip issues: per 16 x 16 tile pair and 256-column chunk ceil(dim / 16) * 4 MFMAs for K, per tile
    pair 4 steps x 2 groups for every 16 columns (rounded up to whole waves of 64), and for RBF the norms once per tile."""
    tiles = (n + 15) // 16
    chunks = (p + 255) // 256
    k_mfma = tiles * tiles * chunks * ((dim + 15) // 16) * 4 + (tiles * ((dim + 15) // 16) * 4 if kind == "rbf" else 0)
    z_mfma = tiles * tiles * ((p + 63) // 64) * 4 * 4 * 2
    return 2048.0 * (k_mfma + z_mfma)                        # a 16 x 16 x 4 MFMA is 1024 multiply-adds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twosample_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")

    def events(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    res = {"device_name": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "fp64_mfma_peak_tflops": FP64_MFMA_PEAK_TFLOPS,
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "torch_host_threads": torch.get_num_threads(), "shapes": {}}
    for n, p, dim in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n + p + dim)
        x = torch.randn(n, dim, device=dev, generator=g)
        x = (x / x.norm(dim=1, keepdim=True)).contiguous()
        labels = torch.randint(0, 3, (n, p), device=dev, generator=g).to(torch.uint8).contiguous()
        xh, lh = x.cpu().numpy(), labels.cpu().numpy()
        for kind, gamma in (("rbf", 1.0), ("poly", 1.0 / dim)):
            routes = {"kernel": lambda: kernel_forms(x, labels, kind=kind, gamma=gamma, coef0=1.0, degree=3),
                      "torch_fp64": lambda: torch_route(x, labels, kind, gamma)}
            for _ in range(WARMUP):
                for fn in routes.values():
                    events(fn, 1)
            calls = 8 if n <= 1024 else 3
            times = {k: [] for k in routes}
            for _ in range(ROUNDS):
                for k, fn in routes.items():
                    times[k].append(events(fn, calls))
            host = []
            for _ in range(HOST_ROUNDS):
                t0 = time.perf_counter()
                ref = numpy_route(xh, lh, kind, gamma)
                host.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            tf = routes["torch_fp64"]()
            torch.cuda.synchronize()
            torch_bytes = torch.cuda.max_memory_allocated(dev) - base
            kf = routes["kernel"]()
            torch.cuda.synchronize()
            scale = tf.abs().max()
            med = {k: statistics.median(v) for k, v in times.items()}
            issued = issued_mfma_flops(n, p, dim, kind)
            useful = 2.0 * n * n * dim + 2.0 * n * n * 2 * p
            key = f"n{n}_p{p}_d{dim}_{kind}"
            res["shapes"][key] = {
                **{k: spread(v) for k, v in times.items()}, "numpy_host": spread(host), "calls_per_sample": calls,
                "torch_fp64_over_kernel": med["torch_fp64"] / med["kernel"],
                "numpy_host_over_kernel": statistics.median(host) / med["kernel"],
                "kernel_issued_mfma_tflops": issued / (med["kernel"] * 1e-3) / 1e12,
                "kernel_fraction_of_fp64_mfma_peak": issued / (med["kernel"] * 1e-3) / 1e12 / FP64_MFMA_PEAK_TFLOPS,
                "kernel_useful_tflops": useful / (med["kernel"] * 1e-3) / 1e12,
                "torch_fp64_useful_tflops": useful / (med["torch_fp64"] * 1e-3) / 1e12,
                "torch_fp64_peak_bytes_allocated": int(torch_bytes),
                "kernel_workspace_bytes": int(_lib.load().siggan_kernel_forms_workspace(n, p)),
                "kernel_output_bytes": 24 * p,
                "max_rel_difference_kernel_vs_torch": float((kf - tf).abs().max() / scale),
                "max_rel_difference_kernel_vs_numpy": float(np.abs(kf.cpu().numpy() - ref).max() / float(scale)),
            }
            print(key, json.dumps(res["shapes"][key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
