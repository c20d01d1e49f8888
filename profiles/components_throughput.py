#!/usr/bin/env python3
"""Time of siggan_components_u8 on the MI355X against the only route the parent has and against a device copy.

    python profiles/components_throughput.py --size 128 --batch 1024 [--out profiles/components_throughput.json]

One run measures one (size, batch) on three inputs that are already on the device and merges its figures into the JSON under
"s<size>_b<batch>", so every shape can run under a time limit of its own:
  "generator"   bytes of a reference_init Generator whose final conv is scaled by 1024 (no trained checkpoint ships with the
                code; a fresh one's bytes are all 127), 256 distinct images repeated
  "noise"       Bernoulli(0.5) ink, the most runs and components a random image has
  "serpentine"  one-pixel columns joined alternately at the top and at the bottom: w / 2 runs in every row, one component
Per input:
  "stats"         components.component_stats, device events around CALLS_PER_SAMPLE back-to-back calls
  "stats_clean"   components.despeckle_u8 with stats into caller-owned outputs (one launch), events likewise
  "copy"          clean.copy_(x) of the same bytes: the floor of anything that reads and writes the images once
  "host"          x.cpu() and a scipy.ndimage.label + bincount loop on ONE thread: a host clock around a call that ends the
                  device work in a synchronise; HOST_ROUNDS rounds (one at batch 16384)
Medians with min and max after WARMUP rounds, the device routes alternating.  The device results are checked against the host
loop's component counts.  Needs the GPU; there is no fallback."""
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
from scipy import ndimage  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import components  # noqa: E402

WARMUP, ROUNDS, CALLS_PER_SAMPLE, HOST_ROUNDS, DISTINCT = 3, 10, 10, 3, 256
EIGHT = np.ones((3, 3), dtype=int)


def generator_bytes(size, dev):
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=100, output_size=size).to(dev).eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
    g._engine.params_changed()
    torch.manual_seed(11)
    return torch.cat([g._engine.g_generate_u8(torch.randn(64, 100, device=dev)) for _ in range(DISTINCT // 64)])


def noise_bytes(size, dev):
    rng = np.random.default_rng(5)
    return torch.from_numpy(np.where(rng.random((DISTINCT, size, size)) < 0.5, 0, 255).astype(np.uint8)).to(dev)


def serpentine_bytes(size, dev):
    g = np.full((size, size), 255, dtype=np.uint8)
    g[:, 0::2] = 0
    for x in range(1, size, 2):
        g[size - 1 if (x >> 1) % 2 == 0 else 0, x] = 0
    return torch.from_numpy(np.broadcast_to(g, (DISTINCT, size, size)).copy()).to(dev)


def tile(x, n):
    return x.repeat((n + x.shape[0] - 1) // x.shape[0], 1, 1)[:n].contiguous()


def host_route(x):
    """-> (components per image, largest area per image): what the parent can do, bytes to the host and scipy per image."""
    host = x.cpu().numpy()
    comps, largest = np.zeros(len(host), np.int64), np.zeros(len(host), np.int64)
    for i, im in enumerate(host):
        lbl, k = ndimage.label(im < 128, structure=EIGHT)
        comps[i] = k
        largest[i] = np.bincount(lbl.ravel())[1:].max() if k else 0
    return comps, largest


def spread(ts):
    return {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_throughput.json"))
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    n, size = a.batch, a.size
    min_area = components.default_min_area(size, size)

    def events(fn, calls=CALLS_PER_SAMPLE):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / calls

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    res = {"device_name": torch.cuda.get_device_name(0), "size": size, "batch": n, "min_area": min_area, "warmup_rounds": WARMUP,
           "calls_per_event_sample": CALLS_PER_SAMPLE, "host_threads": 1, "inputs": {}}
    for name, make in (("generator", generator_bytes), ("noise", noise_bytes), ("serpentine", serpentine_bytes)):
        x = tile(make(size, dev), n)
        stats = torch.empty(n, 9, dtype=torch.int32, device=dev)
        clean = torch.empty_like(x)
        routes = {"stats": lambda: components.component_stats(x, 128, 8, min_area),
                  "stats_clean": lambda: components.despeckle_u8(x, 128, 8, min_area, out=clean, stats=stats),
                  "copy": lambda: clean.copy_(x)}
        for _ in range(WARMUP):
            for fn in routes.values():
                events(fn, 2)
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                times[k].append(events(fn))
        host_rounds = 1 if n > 4096 else HOST_ROUNDS
        clock(lambda: host_route(x[:min(n, 64)]))                                    # warm-up on a few images
        host_times, host_out = [], None
        for _ in range(host_rounds):
            t, host_out = clock(lambda: host_route(x))
            host_times.append(t)
        components.despeckle_u8(x, 128, 8, min_area, out=clean, stats=stats)
        s = stats.cpu().numpy()
        med = {k: statistics.median(v) for k, v in times.items()}
        host_med = statistics.median(host_times)
        res["inputs"][name] = {
            **{k: spread(v) for k, v in times.items()}, "host": spread(host_times),
            "stats_ns_per_image": 1e9 * med["stats"] / n, "stats_clean_ns_per_image": 1e9 * med["stats_clean"] / n,
            "host_us_per_image": 1e6 * host_med / n,
            "stats_over_copy": med["stats"] / med["copy"], "stats_clean_over_copy": med["stats_clean"] / med["copy"],
            "host_over_stats": host_med / med["stats"], "host_over_stats_clean": host_med / med["stats_clean"],
            "components_mean": float(s[:, components.COMPONENTS].mean()), "ink_mean": float(s[:, components.INK].mean()),
            "bound_never_hit": bool((s[:, components.COMPONENTS] >= 0).all()),
            "device_equals_host_counts": bool(np.array_equal(s[:, components.COMPONENTS], host_out[0])
                                              and np.array_equal(s[:, components.LARGEST], host_out[1]))}
        print(name, json.dumps(res["inputs"][name]), flush=True)
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[f"s{size}_b{n}"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
