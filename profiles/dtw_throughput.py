#!/usr/bin/env python3
"""Pairs per second of siggan_dtw_pairs on the MI355X against the same recurrence written with torch ops on the same device.

    python profiles/dtw_throughput.py [--out profiles/dtw_throughput.json]

2048 x 2048 pairs of column profiles at w = 64 (band 8) and w = 128 (band 16), the default bands.  The profiles come from
seeded random byte images with a tenth of their pixels inked (the kernel's work does not depend on the values).  Per width:
  "kernel_matrix"  dtw.dtw_matrix of two prepared DtwSets: one launch that writes the (2048, 2048) int32 matrix
  "kernel_best"    dtw.dtw_best of the same sets: the same pairs, no matrix, one key per row and slice of columns
  "torch"          the yardstick: the banded recurrence as 2 w - 1 anti-diagonal steps of elementwise torch ops (subtract,
                   abs, sum over the four bytes, two minimums, add, slice assignment) over int32 tensors with one row per
                   pair -- (na * nb, w + 1) per diagonal, three diagonals kept --, TORCH_ROWS rows of a at a time to bound
                   the memory; a step touches only the columns inside the band.  Its matrix must equal the kernel's.
WARMUP calls of every route, then ROUNDS samples per route, the routes alternating.  A sample is device events around
CALLS[route] back-to-back calls, divided by their number.  Medians with min and max of the time per call, pairs per second
from the median and the ratio torch / kernel.  There is no pass / fail threshold.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import dtw  # noqa: E402

WARMUP, ROUNDS, N, TORCH_ROWS = 1, 5, 2048, 128
CALLS = {"kernel_matrix": 20, "kernel_best": 20, "torch": 1}
BIG = 1 << 30


def torch_dtw(pa, pb, band, rows=TORCH_ROWS):
    """int32 (na, nb): banded DTW of every profile of pa (na, w, 4) uint8 with every profile of pb, torch ops only."""
    na, w = pa.shape[0], pa.shape[1]
    nb = pb.shape[0]
    out = torch.empty((na, nb), dtype=torch.int32, device=pa.device)
    b = pb.to(torch.int32)
    for r0 in range(0, na, rows):
        a = pa[r0:r0 + rows].to(torch.int32)
        n = a.shape[0]
        a = a[:, None].expand(n, nb, w, 4).reshape(n * nb, w, 4)
        bb = b[None].expand(n, nb, w, 4).reshape(n * nb, w, 4)
        # diagonal s holds cell (i, s - i) at index i + 1; index 0 and everything outside the band is BIG
        two_back = torch.full((n * nb, w + 1), BIG, dtype=torch.int32, device=pa.device)
        one_back, now = two_back.clone(), two_back.clone()
        two_back[:, 0] = 0                                               # D(-1, -1) = 0 makes D(0, 0) = d(0, 0)
        for s in range(2 * w - 1):
            i0 = max(0, s - w + 1, (s - band + 1) // 2)
            i1 = min(w - 1, s, (s + band) // 2)
            now.fill_(BIG)
            cost = (a[:, i0:i1 + 1] - bb[:, s - i1:s - i0 + 1].flip(1)).abs().sum(-1)
            best = torch.minimum(torch.minimum(one_back[:, i0:i1 + 1], one_back[:, i0 + 1:i1 + 2]), two_back[:, i0:i1 + 1])
            now[:, i0 + 1:i1 + 2] = cost + best
            two_back, one_back, now = one_back, now, two_back
        out[r0:r0 + n] = one_back[:, w].reshape(n, nb)
    return out


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dtw_throughput.json"))
    ap.add_argument("--n", type=int, default=N, help="images per set (the recorded numbers are at 2048)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")

    def events(fn, calls=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    res = {"device_name": torch.cuda.get_device_name(0), "images_per_set": a.n, "pairs": a.n * a.n, "warmup_calls": WARMUP,
           "calls_per_sample": CALLS, "torch_rows_per_chunk": TORCH_ROWS, "widths": {}}
    for w in (64, 128):
        band = dtw.default_band(w)
        gen = torch.Generator(device=dev).manual_seed(w)
        images = [torch.where(torch.rand((a.n, w, w), device=dev, generator=gen) < 0.1, 0, 255).to(torch.uint8) for _ in range(2)]
        sa, sb = dtw.DtwSet(images[0]), dtw.DtwSet(images[1])
        routes = {"kernel_matrix": lambda: dtw.dtw_matrix(sa, sb, band), "kernel_best": lambda: dtw.dtw_best(sa, sb, band),
                  "torch": lambda: torch_dtw(sa.profiles, sb.profiles, band)}
        for _ in range(WARMUP):
            for fn in routes.values():
                events(fn)
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                times[k].append(events(fn, CALLS[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        matrix = dtw.dtw_matrix(sa, sb, band)
        same = bool(torch.equal(matrix, torch_dtw(sa.profiles, sb.profiles, band)))
        best, index = dtw.dtw_best(sa, sb, band)
        same_best = bool(torch.equal(best, matrix.min(dim=1).values))
        res["widths"][f"w{w}"] = {
            "band": band, **{k: spread(v) for k, v in times.items()},
            **{f"{k}_pairs_per_s": a.n * a.n / (1e-3 * med[k]) for k in routes},
            "torch_over_kernel_matrix": med["torch"] / med["kernel_matrix"], "torch_over_kernel_best": med["torch"] / med["kernel_best"],
            "matrix_equals_torch": same, "best_equals_matrix_minimum": same_best}
        print(w, json.dumps(res["widths"][f"w{w}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
