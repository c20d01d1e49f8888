#!/usr/bin/env python3
"""Time of k-means++ seeding and of Lloyd passes (siggan_kmeans_seed, siggan_kmeans_lloyd) on the MI355X against the same
loops written with torch ops on the same device.

    python profiles/kmeans_throughput.py [--out profiles/kmeans_throughput.json]

Pools (fp32, resident on the device): 100 normal blobs, means 4 * N(0, 1) per feature, unit variance.  Per shape
(n, dim, k) = (20000, 128, 100) and (20000, 1024, 100):
  "seed"          utils.modes.seed_centres: 2 k - 1 launches enqueued blindly
  "lloyd20"       20 Lloyd passes and the final assignment from those centres (siggan_kmeans_lloyd, iterations = 20; the copy
                  of the start centres is inside the sample): four launches per pass
  "torch_*_seed"  D^2 sampling with torch ops, no host decision per centre: index_select of the last pick, squared distances
                  as ((x - c) ** 2).sum(1), torch.minimum, cumsum, searchsorted of u * total (u from torch.rand)
  "torch_*_lloyd20"  per pass torch.cdist, argmin, index_add_ of the rows into zeroed sums, bincount, a guarded division;
                  then the final cdist / argmin / inertia.  index_add_ adds with atomics: its sums are not reproducible
  fp32: on the pool as it is (what one would write without the fp64 contract; not the same numbers); fp64: on the pool
  widened beforehand.
The worst case of the centre update -- every row in one centre, n = 65536, dim = 1024, k = 2 with the second centre far away
-- is timed as the call with iterations = 1 (assign, update, assign) beside the call with iterations = 0 (assign, with its
counters); "update_ms" is the first minus twice the second.

WARMUP calls per route, then ROUNDS samples per route, the routes alternating.  A sample is device events around as many
back-to-back calls as fill about TARGET_MS of device time (from the warm-up's own timing), divided by their number.  Medians
with min and max.  "inertia_rel_diff_to_torch_fp64": the two fp64 routes' final inertia from the same start centres (the torch
route sums in another order, and its labels may differ where two centres are equally near).  There is no pass / fail
threshold.  Needs the GPU; there is no fallback."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import _lib  # noqa: E402
from signature_gan_amd.utils import modes  # noqa: E402

WARMUP, ROUNDS, TARGET_MS, PASSES = 2, 7, 200.0, 20
SHAPES = [(20000, 128, 100), (20000, 1024, 100)]
WORST = (65536, 1024, 2)


def pool(n, dim, blobs, dev):
    g = torch.Generator(device=dev).manual_seed(n + dim)
    means = 4.0 * torch.randn(blobs, dim, device=dev, generator=g)
    which = torch.randint(0, blobs, (n,), device=dev, generator=g)
    return (means[which] + torch.randn(n, dim, device=dev, generator=g)).contiguous()


def torch_seed(x, k, u):
    """k-means++ with torch ops; u (k,) uniforms on the device.  -> the (k, dim) centres."""
    n = x.shape[0]
    rows = torch.empty(k, dtype=torch.int64, device=x.device)
    rows[0:1] = (u[0:1] * n).long().clamp_(max=n - 1)
    m = torch.full((n,), float("inf"), dtype=x.dtype, device=x.device)
    for s in range(1, k):
        m = torch.minimum(m, ((x - x.index_select(0, rows[s - 1:s])) ** 2).sum(1))
        prefix = torch.cumsum(m, 0)
        rows[s:s + 1] = torch.searchsorted(prefix, u[s:s + 1] * prefix[-1:], right=True).clamp_(max=n - 1)
    return x.index_select(0, rows)


def torch_lloyd(x, centres, passes):
    """-> (centres, labels, inertia) after ``passes`` updates and a final assignment."""
    k = centres.shape[0]
    for _ in range(passes):
        labels = torch.cdist(x, centres).argmin(1)
        sums = torch.zeros_like(centres).index_add_(0, labels, x)
        counts = torch.bincount(labels, minlength=k)
        centres = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None].to(x.dtype), centres)
    d, labels = torch.cdist(x, centres).min(1)
    return centres, labels, (d * d).sum()


def lloyd_call(x, centres, iterations):
    dev = x.device
    lib = _lib.load()
    workspace, size = modes._workspace(lib, x.shape[0], x.shape[1], centres.shape[0], dev)
    return lambda: modes._lloyd(lib, x, centres.clone(), iterations, dev, workspace, size)


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)}


def events(fn, calls=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(routes):
    """{route: spread} and the calls per sample; the routes alternate inside every round."""
    calls = {}
    for name, fn in routes.items():
        one = min(events(fn) for _ in range(WARMUP))
        calls[name] = max(1, min(2000, math.ceil(TARGET_MS / max(one, 1e-3))))
    times = {name: [] for name in routes}
    for _ in range(ROUNDS):
        for name, fn in routes.items():
            times[name].append(events(fn, calls[name]))
    return {name: spread(ts) for name, ts in times.items()}, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device_name": torch.cuda.get_device_name(0), "warmup_calls": WARMUP, "rounds": ROUNDS, "target_ms_per_sample": TARGET_MS,
           "passes": PASSES, "shapes": {}}
    for n, dim, k in SHAPES:
        x = pool(n, dim, k, dev)
        x64 = x.double()
        start, _ = modes.seed_centres(x, k, 0)
        start64 = start.double()
        u32 = torch.rand(k, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        u64 = u32.double()
        routes = {"seed": lambda: modes.seed_centres(x, k, 0), "lloyd20": lloyd_call(x, start, PASSES),
                  "torch_fp32_seed": lambda: torch_seed(x, k, u32), "torch_fp32_lloyd20": lambda: torch_lloyd(x, start, PASSES),
                  "torch_fp64_seed": lambda: torch_seed(x64, k, u64), "torch_fp64_lloyd20": lambda: torch_lloyd(x64, start64, PASSES)}
        out, calls = measure(routes)
        med = {name: v["median_ms"] for name, v in out.items()}
        _, _, _, inertia, changed = lloyd_call(x, start, PASSES)()
        t_inertia = float(torch_lloyd(x64, start64, PASSES)[2].item())
        k_inertia = float(inertia[-1].item())
        out.update({"calls_per_sample": calls, "changed_per_pass": changed.cpu().tolist(),
                    "inertia_rel_diff_to_torch_fp64": abs(k_inertia - t_inertia) / t_inertia,
                    "lloyd_ms_per_pass": med["lloyd20"] / (PASSES + 1)})
        for kind in ("seed", "lloyd20"):
            for prec in ("fp32", "fp64"):
                out[f"torch_{prec}_over_kernel_{kind}"] = med[f"torch_{prec}_{kind}"] / med[kind]
        res["shapes"][f"n{n}_dim{dim}_k{k}"] = out
        print(n, dim, k, json.dumps(out), flush=True)

    n, dim, k = WORST
    x = pool(n, dim, 1, dev)
    centres = torch.cat([x.mean(0, keepdim=True), torch.full((1, dim), 1e4, device=dev)]).contiguous()
    out, calls = measure({"assign_ms": lloyd_call(x, centres, 0), "assign_update_assign_ms": lloyd_call(x, centres, 1)})
    counts = lloyd_call(x, centres, 1)()[2].cpu().tolist()
    assert counts == [n, 0], counts
    out.update({"calls_per_sample": calls, "counts": counts,
                "update_ms": out["assign_update_assign_ms"]["median_ms"] - 2 * out["assign_ms"]["median_ms"]})
    res["worst_case_one_centre"] = {f"n{n}_dim{dim}_k{k}": out}
    print("worst", json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
