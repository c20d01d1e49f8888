#!/usr/bin/env python3
"""Time of the device resize on the MI355X against the host route it replaces.

    python profiles/resize_throughput.py --batch 64 [--out profiles/resize_throughput.json]
    python profiles/resize_throughput.py --batch 1024
    python profiles/resize_throughput.py --batch 16384 --resize_only

One run measures one batch of 128x128 uint8 images that are already on the device (stroke-like bytes) and merges its
figures into the JSON under the key "batch_<n>", so every batch can run under a time limit of its own:
  "resize_u8"          resize.resize_u8 into a caller-owned output, device events around CALLS_PER_SAMPLE back-to-back calls
  "embed_u8_64"        SiameseNetwork.embed_u8 of the resized bytes (what a 64x64 Generator's batch costs), events likewise
  "embed_resized_128"  SiameseNetwork.embed_resized of the 128x128 bytes: the two above in one call; the difference is the
                       share the resize adds
  "host_route"         device -> host, Image.resize per image, host -> device; host clock around a call that ends in a
                       synchronise
Five warm-up rounds, then 20 timed rounds alternating between the routes; medians with min and max.  resize_u8 reads
16 KiB and writes 4 KiB per image: its bytes over its time are set against the measured copy bandwidth of HBM (6.29 TB/s,
a float4 copy) -- but a batch of 1024 is 20 MiB and lives in the 256 MiB Infinity Cache, so only a batch whose input alone
exceeds it (--batch 16384: 256 MiB in) says something about HBM.  The verifier has random weights (speed does not depend on
them).  Needs the GPU; there is no fallback."""
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
from PIL import Image  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd.resize import resize_u8  # noqa: E402
from signature_gan_amd.signature_verifier_eval import SiameseNetwork  # noqa: E402

SIZE, OUT, WARMUP, ROUNDS, CALLS_PER_SAMPLE = 128, 64, 5, 20, 20
HBM_COPY_TBS = 6.29                                          # measured float4 copy on the MI355X
INFINITY_CACHE_BYTES = 256 << 20


def stroke_bytes(n, seed):
    """White pages with dark noise along a few rows: compressible like a signature, different per image."""
    rng = np.random.default_rng(seed)
    a = np.full((n, SIZE, SIZE), 255, dtype=np.uint8)
    rows = rng.integers(8, SIZE - 8, size=(n, 6))
    for i in range(min(n, 256)):                             # 256 distinct images, repeated: content does not change the time
        for r in rows[i]:
            a[i, r:r + 2, 10:SIZE - 10] = rng.integers(0, 160, size=(2, SIZE - 20), dtype=np.uint8)
    for i in range(256, n):
        a[i] = a[i % 256]
    return a


def pillow_route(x):
    host = x.cpu().numpy()
    small = np.stack([np.asarray(Image.fromarray(im).resize((OUT, OUT), Image.BILINEAR), dtype=np.uint8) for im in host])
    return torch.from_numpy(small).to(x.device)


def spread(ts):
    return {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts), "samples": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_throughput.json"))
    ap.add_argument("--batch", type=int, required=True)
    ap.add_argument("--resize_only", action="store_true", help="time resize_u8 alone (batches beyond what the verifier and the host route are asked)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    n = a.batch
    x = torch.from_numpy(stroke_bytes(n, 1)).to(dev)
    small = torch.empty(n, OUT, OUT, dtype=torch.uint8, device=dev)

    def events(fn, calls=CALLS_PER_SAMPLE):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / calls, out

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    routes = {"resize_u8": (events, lambda: resize_u8(x, OUT, out=small))}
    if not a.resize_only:
        model = SiameseNetwork(128, max_images=n).to(dev).eval()
        routes["embed_u8_64"] = (events, lambda: model.embed_u8(small))
        routes["embed_resized_128"] = (events, lambda: model.embed_resized(x))
        routes["host_route"] = (clock, lambda: pillow_route(x))
    last = {}
    for name, (timer, fn) in routes.items():
        for _ in range(WARMUP):
            last[name] = timer(fn)[1]
    times = {name: [] for name in routes}
    for _ in range(ROUNDS):
        for name, (timer, fn) in routes.items():
            times[name].append(timer(fn)[0])

    t = statistics.median(times["resize_u8"])
    moved = n * (SIZE * SIZE + OUT * OUT)
    res = {"device_name": torch.cuda.get_device_name(0), "batch": n, "warmup_rounds": WARMUP, "calls_per_event_sample": CALLS_PER_SAMPLE,
           "resize_u8": spread(times["resize_u8"]), "resize_u8_bytes_moved": moved, "resize_u8_tb_per_s": moved / t * 1e-12,
           "resize_u8_fraction_of_hbm_copy_bandwidth": moved / t * 1e-12 / HBM_COPY_TBS,
           "working_set_fits_infinity_cache": bool(moved <= INFINITY_CACHE_BYTES),
           "resize_u8_images_per_s": n / t,
           "resize_u8_bit_equal_rerun": bool(torch.equal(resize_u8(x, OUT), small))}
    if not a.resize_only:
        e64, e128 = statistics.median(times["embed_u8_64"]), statistics.median(times["embed_resized_128"])
        res.update({"embed_u8_64": spread(times["embed_u8_64"]), "embed_resized_128": spread(times["embed_resized_128"]),
                    "resize_share_of_embed_resized": (e128 - e64) / e128,
                    "host_route": spread(times["host_route"]),
                    "host_route_over_resize_u8_median": statistics.median(times["host_route"]) / t,
                    "host_route_equals_device_bytes": bool(torch.equal(last["host_route"], small))})
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[f"batch_{n}"] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(merged, f, indent=2, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
