#!/usr/bin/env python3
"""Time of siggan_strokes_u8 on the MI355X against the only route the parent has and against a device copy.

    python profiles/strokes_throughput.py --size 128 --batch 1024 [--out profiles/strokes_throughput.json]

One run measures one (size, batch) on three inputs that are already on the device and merges its figures into the JSON under
"s<size>_b<batch>", so every shape can run under a time limit of its own:
  "generator"   bytes of a reference_init Generator whose final conv is scaled by 1024 (no trained checkpoint ships with the
                code; a fresh one's bytes are all 127), 256 distinct images repeated
  "noise"       Bernoulli(0.5) ink
  "full"        every pixel ink: the most thinning passes an image of the size needs (size / 2 + 1) and the longest row searches
                of the distance map
Per input:
  "stats"       strokes.stroke_stats, device events around CALLS_PER_SAMPLE back-to-back calls
  "all"         one launch with all four outputs (counters, distance map, skeleton, redraw at radius^2 4) into caller-owned
                buffers, events likewise
  "copy"        out.copy_(x) of the same bytes: the floor of anything that reads and writes the images once
  "host"        x.cpu(), then scipy.ndimage.distance_transform_edt and a numpy Guo-Hall thinning per image on ONE thread: a host
                clock around a call that ends the device work in a synchronise.  The numpy thinning takes milliseconds per image,
                so the host route runs on the first HOST_IMAGES images only and is reported per image
Medians with min and max after WARMUP rounds, the device routes alternating.  The device's counters are checked against the
host route's skeleton lengths and largest distances.  Needs the GPU; there is no fallback."""
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
from signature_gan_amd import strokes  # noqa: E402

WARMUP, ROUNDS, CALLS_PER_SAMPLE, HOST_ROUNDS, HOST_IMAGES, DISTINCT, RADIUS2 = 3, 10, 10, 3, 64, 256, 4


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


def full_bytes(size, dev):
    return torch.zeros((DISTINCT, size, size), dtype=torch.uint8, device=dev)


def tile(x, n):
    return x.repeat((n + x.shape[0] - 1) // x.shape[0], 1, 1)[:n].contiguous()


def thin(mask):
    """Guo-Hall A1 on a boolean image, the paper going on beyond the border -> skeleton."""
    m = np.pad(mask, 1)
    while True:
        changed = False
        for sub in (0, 1):
            p2, p6, p4, p8 = np.roll(m, 1, 0), np.roll(m, -1, 0), np.roll(m, -1, 1), np.roll(m, 1, 1)
            p3, p9, p5, p7 = np.roll(p2, -1, 1), np.roll(p2, 1, 1), np.roll(p6, -1, 1), np.roll(p6, 1, 1)
            c = (~p2 & (p3 | p4)).astype(np.int8) + (~p4 & (p5 | p6)) + (~p6 & (p7 | p8)) + (~p8 & (p9 | p2))
            n = np.minimum((p9 | p2).astype(np.int8) + (p3 | p4) + (p5 | p6) + (p7 | p8),
                           (p2 | p3).astype(np.int8) + (p4 | p5) + (p6 | p7) + (p8 | p9))
            delete = m & (c == 1) & (n >= 2) & (n <= 3) & ~(((p2 | p3 | ~p5) & p4) if sub == 0 else ((p6 | p7 | ~p9) & p8))
            if delete.any():
                changed, m = True, m & ~delete
        if not changed:
            return m[1:-1, 1:-1]


def host_route(x):
    """-> (skeleton pixels per image, largest squared distance per image): bytes to the host, scipy and numpy per image."""
    host = x.cpu().numpy()
    length, d2_max = np.zeros(len(host), np.int64), np.zeros(len(host), np.int64)
    for i, im in enumerate(host):
        mask = im < 128
        d = ndimage.distance_transform_edt(np.pad(mask, 1))
        length[i] = thin(mask).sum()
        d2_max[i] = int(np.rint(d.max() ** 2))
    return length, d2_max


def spread(ts):
    return {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strokes_throughput.json"))
    ap.add_argument("--size", type=int, required=True)
    ap.add_argument("--batch", type=int, required=True)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    n, size = a.batch, a.size
    host_n = min(n, HOST_IMAGES)

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

    lib = signature_gan_amd._lib.load()
    res = {"device_name": torch.cuda.get_device_name(0), "size": size, "batch": n, "radius2": RADIUS2, "warmup_rounds": WARMUP,
           "calls_per_event_sample": CALLS_PER_SAMPLE, "host_threads": 1, "host_images": host_n, "inputs": {}}
    for name, make in (("generator", generator_bytes), ("noise", noise_bytes), ("full", full_bytes)):
        x = tile(make(size, dev), n)
        stats = torch.empty(n, strokes.COUNT, dtype=torch.int32, device=dev)
        d2 = torch.empty(x.shape, dtype=torch.int16, device=dev)
        skel, redraw = torch.empty_like(x), torch.empty_like(x)
        stream = torch.cuda.current_stream().cuda_stream

        def all_outputs():
            signature_gan_amd._lib.check(lib.siggan_strokes_u8(0, x.data_ptr(), n, size, size, 128, RADIUS2, 0, 255, stats.data_ptr(),
                                                               d2.data_ptr(), skel.data_ptr(), redraw.data_ptr(), stream))

        routes = {"stats": lambda: strokes.stroke_stats(x), "all": all_outputs, "copy": lambda: redraw.copy_(x)}
        for _ in range(WARMUP):
            for fn in routes.values():
                events(fn, 2)
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                times[k].append(events(fn))
        clock(lambda: host_route(x[:4]))                                             # warm-up on a few images
        host_times, host_out = [], None
        for _ in range(HOST_ROUNDS):
            t, host_out = clock(lambda: host_route(x[:host_n]))
            host_times.append(t)
        all_outputs()
        s = stats.cpu().numpy()
        med = {k: statistics.median(v) for k, v in times.items()}
        host_per_image = statistics.median(host_times) / host_n
        res["inputs"][name] = {
            **{k: spread(v) for k, v in times.items()}, "host": spread(host_times),
            "stats_ns_per_image": 1e9 * med["stats"] / n, "all_ns_per_image": 1e9 * med["all"] / n,
            "host_us_per_image": 1e6 * host_per_image,
            "stats_over_copy": med["stats"] / med["copy"], "all_over_copy": med["all"] / med["copy"],
            "host_over_stats": host_per_image * n / med["stats"], "host_over_all": host_per_image * n / med["all"],
            "passes_max": int(s[:, strokes.PASSES].max()), "skeleton_mean": float(s[:, strokes.SKELETON].mean()),
            "ink_mean": float(s[:, strokes.INK].mean()), "bound_never_hit": bool((s[:, strokes.PASSES] >= 1).all()),
            "device_equals_host_counts": bool(np.array_equal(s[:host_n, strokes.SKELETON], host_out[0])
                                              and np.array_equal(s[:host_n, strokes.D2_MAX], host_out[1]))}
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
