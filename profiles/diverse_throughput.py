#!/usr/bin/env python3
"""Time of siggan_select_diverse on the MI355X against the same greedy loop written with torch ops on the same device.

    python profiles/diverse_throughput.py [--out profiles/diverse_throughput.json]

Pools of 4096 and 16384 rows of dim 128 (standard normal, fp32, already on the device), n_select 256 and 1024, no mask, no
anchors, min_separation 0.  Per shape:
  "kernel"      utils.diverse.select_diverse: n_select + 2 launches enqueued blindly
  "torch_fp64"  the yardstick: per pick a masked argmax whose index stays on the device, index_select of that row, a row of
                squared distances as ((x64 - row) ** 2).sum(1) on a pool widened to fp64 beforehand, torch.minimum into m --
                no host decision per pick either
  "torch_fp32"  the same loop on the fp32 pool: what one would write without the fp64 contract (it does not compute the
                same numbers)
WARMUP whole selections, then ROUNDS samples per route, the routes alternating.  A sample is device events around
PICKS_PER_SAMPLE[route] / n_select back-to-back selections -- about a fifth to a quarter of a second of device time per
sample -- divided by their number.  Medians with min and max of the time per selection, the time per pick (selection /
n_select) and the ratio torch / kernel.  "same_picks_as_torch_fp64" records whether the two fp64 routes
chose the same rows.  There is no pass / fail threshold.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd.utils.diverse import select_diverse  # noqa: E402

WARMUP, ROUNDS, DIM = 2, 7, 128
PICKS_PER_SAMPLE = {"kernel": 20480, "torch_fp64": 5120, "torch_fp32": 5120}     # about 0.2 s and 0.25 s of device time
SHAPES = [(4096, 256), (4096, 1024), (16384, 256), (16384, 1024)]


def torch_loop(x, n_select):
    """Greedy farthest-point picks with torch ops only; x (n, dim) fp32 or fp64.  Returns the int64 (n_select,) picks."""
    n = x.shape[0]
    m = torch.full((n,), float("inf"), dtype=x.dtype, device=x.device)
    avail = torch.ones(n, dtype=torch.bool, device=x.device)
    low = torch.full((n,), -1.0, dtype=x.dtype, device=x.device)
    order = torch.empty(n_select, dtype=torch.int64, device=x.device)
    for t in range(n_select):
        p = torch.argmax(torch.where(avail, m, low)).view(1)             # the first of equal maxima
        order[t:t + 1] = p
        avail.index_fill_(0, p, False)
        d = ((x - x.index_select(0, p)) ** 2).sum(1)
        m = torch.minimum(m, d)
    return order


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_throughput.json"))
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

    res = {"device_name": torch.cuda.get_device_name(0), "dim": DIM, "warmup_selections": WARMUP, "shapes": {}}
    for n, n_select in SHAPES:
        x = torch.randn(n, DIM, device=dev, generator=torch.Generator(device=dev).manual_seed(n))
        x64 = x.double()
        routes = {"kernel": lambda: select_diverse(x, n_select), "torch_fp64": lambda: torch_loop(x64, n_select),
                  "torch_fp32": lambda: torch_loop(x, n_select)}
        for _ in range(WARMUP):
            for fn in routes.values():
                events(fn)
        calls = {k: max(1, PICKS_PER_SAMPLE[k] // n_select) for k in routes}
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                times[k].append(events(fn, calls[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        same = bool(torch.equal(select_diverse(x, n_select)[0].long(), torch_loop(x64, n_select)))
        res["shapes"][f"n{n}_k{n_select}"] = {
            **{k: spread(v) for k, v in times.items()},
            **{f"{k}_us_per_pick": 1e3 * med[k] / n_select for k in routes},
            "torch_fp64_over_kernel": med["torch_fp64"] / med["kernel"], "torch_fp32_over_kernel": med["torch_fp32"] / med["kernel"],
            "selections_per_sample": calls, "same_picks_as_torch_fp64": same}
        print(n, n_select, json.dumps(res["shapes"][f"n{n}_k{n_select}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
