#!/usr/bin/env python3
"""Time of the nearest-neighbour metrics on the MI355X against the route a user has without them.

    python profiles/neighbors_throughput.py [--out profiles/neighbors_throughput.json] [--n 10000]

n_real = n_fake = n unit-norm rows of dim 128 (what the verifier's embeddings look like), k = 3:
  "knn"       one siggan_knn launch, n x n, device events around each launch
  "manifold"  utils.neighbors.manifold_metrics: six launches, the copies of k-lists and counts, the numpy reduction;
              host clock, every call ends in device-to-host copies and hence in a synchronise
  baseline    the same answers from torch on the same GPU: torch.cdist on .double() inputs, chunked over the queries so that
              a chunk's fp64 distance block stays under 256 MiB, then topk(k, largest=False) / comparisons against the radii
Five warm-up calls each, then 20 timed calls alternating between the routes; medians with min and max.  The fused kernel's
fraction of the fp64 MFMA peak counts the 2 n^2 dim flops of the dot products only -- the kernel issues twice as many
(the reference norms run through the MFMA as well, include/siggan_neighbors.h), so its MFMA pipe is twice as busy as the
fraction says.  The baseline's neighbours are compared with the kernel's: row numbers may differ where cdist's fp64 result
differs from the exact one by more than a gap, and the script reports how many do.  Needs the GPU; there is no fallback."""
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
from signature_gan_amd.utils.neighbors import knn, manifold_from_neighbors, manifold_metrics  # noqa: E402

DIM, K, WARMUP, CALLS = 128, 3, 5, 20
FP64_MFMA_PEAK_TFLOPS = 78.6                                 # MI355X, matrix fp64 (AMD's product brief)
BLOCK_BYTES = 256 << 20


def unit_rows(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, DIM, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().to(dev).contiguous()


def chunk_rows(n_ref):
    return max(1, BLOCK_BYTES // (8 * n_ref))


def torch_knn(q, r, k, exclude_self=False):
    qd, rd = q.double(), r.double()
    d2s, idxs = [], []
    step = chunk_rows(r.shape[0])
    for lo in range(0, q.shape[0], step):
        d = torch.cdist(qd[lo:lo + step], rd)
        if exclude_self:
            rows = torch.arange(d.shape[0], device=d.device)
            d[rows, rows + lo] = float("inf")
        v, i = torch.topk(d, k, dim=1, largest=False)
        d2s.append(v * v), idxs.append(i)
    return torch.cat(d2s), torch.cat(idxs)


def torch_ball_count(q, r, radius2):
    qd, rd = q.double(), r.double()
    out = []
    step = chunk_rows(r.shape[0])
    for lo in range(0, q.shape[0], step):
        d = torch.cdist(qd[lo:lo + step], rd)
        out.append(((d * d) <= radius2[None, :]).sum(dim=1))
    return torch.cat(out)


def torch_manifold(real, fake, k):
    real_d2, _ = torch_knn(real, real, k, True)
    fake_d2, _ = torch_knn(fake, fake, k, True)
    rr, rf = real_d2[:, k - 1].contiguous(), fake_d2[:, k - 1].contiguous()
    fake_in_real, real_in_fake = torch_ball_count(fake, real, rr), torch_ball_count(real, fake, rf)
    r2f, _ = torch_knn(real, fake, 1)
    f2r, f2r_i = torch_knn(fake, real, 1)
    host = [t.cpu().numpy() for t in (rr, rf, fake_in_real, real_in_fake, r2f, f2r, f2r_i, real_d2[:, 0])]
    return manifold_from_neighbors(k, *host)


def spread(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "calls": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors_throughput.json"))
    ap.add_argument("--n", type=int, default=10000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    n = a.n
    real, fake = unit_rows(n, 1, dev), unit_rows(n, 2, dev)

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3, out

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    routes = {"knn": (events, lambda: knn(fake, real, K)), "knn_torch": (events, lambda: torch_knn(fake, real, K)),
              "manifold": (clock, lambda: manifold_metrics(real, fake, K)), "manifold_torch": (clock, lambda: torch_manifold(real, fake, K))}
    last = {}
    for name, (timer, fn) in routes.items():
        for _ in range(WARMUP):
            last[name] = timer(fn)[1]
    times = {name: [] for name in routes}
    for _ in range(CALLS):
        for name, (timer, fn) in routes.items():
            times[name].append(timer(fn)[0])

    (d2, idx), (d2_t, idx_t) = last["knn"], last["knn_torch"]
    index_mismatch = int((idx.long() != idx_t).sum())
    worst_d2_diff = float((d2 - d2_t).abs().max())
    again = knn(fake, real, K)
    m, m_t = last["manifold"], last["manifold_torch"]
    knn_s = statistics.median(times["knn"])
    tflops = 2.0 * n * n * DIM / knn_s * 1e-12
    out = {"device_name": torch.cuda.get_device_name(0), "n_real": n, "n_fake": n, "dim": DIM, "k": K, "warmup": WARMUP,
           "knn": spread(times["knn"]), "knn_torch_cdist_topk": spread(times["knn_torch"]),
           "knn_speedup_median": statistics.median(times["knn_torch"]) / knn_s,
           "knn_dot_tflops": tflops, "knn_fraction_of_fp64_mfma_peak": tflops / FP64_MFMA_PEAK_TFLOPS,
           "knn_bit_equal_rerun": bool(torch.equal(again[0], d2) and torch.equal(again[1], idx)),
           "knn_vs_torch": {"row_numbers_that_differ": index_mismatch, "of": int(idx.numel()), "worst_d2_difference": worst_d2_diff},
           "manifold": spread(times["manifold"]), "manifold_torch": spread(times["manifold_torch"]),
           "manifold_speedup_median": statistics.median(times["manifold_torch"]) / statistics.median(times["manifold"]),
           "manifold_figures": {key: m[key] for key in ("precision", "recall", "density", "coverage")},
           "manifold_figures_torch": {key: m_t[key] for key in ("precision", "recall", "density", "coverage")},
           "distance_matrix_bytes_not_written": 8 * n * n, "knn_output_bytes": 12 * n * K}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
