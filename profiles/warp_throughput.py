#!/usr/bin/env python3
"""Images per second of warp.warp_u8 on the MI355X, beside the same warp written in torch ops on the same GPU.

    python profiles/warp_throughput.py [--out profiles/warp_throughput.json]

2048 byte images (eight distinct stroke images repeated), pool resident, at 64 x 64 with cell 16 and at 128 x 128 with cell
32, amplitude 0.4 cells, identity base map.  Per size:
  "hip"    one siggan_warp_u8 launch through warp.warp_u8 into a caller-owned tensor (the call uploads its 2048 parameter
           rows, as every user's call does): device events around CALLS calls, ROUNDS rounds after WARMUP, per-call time
           from the median round
  "hip_resident_rows"  the same launch through the C ABI with the parameter rows already on the device
  "torch"  the same warp in torch ops: random control points (torch.rand on the device), the dense displacement as two
           matrix products with the cubic B-spline weight matrices, torch.nn.functional.grid_sample (bilinear,
           align_corners=True) on the fp32 image, rounded back to bytes.  Its random numbers and its rounding are its own,
           so only its time is compared, not its bytes.
The first image's bytes are checked against the numpy restatement (tests/warpcommon.py).  No pass / fail threshold.  Needs
the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import warpcommon as W  # noqa: E402
import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import _call, _lib, warp  # noqa: E402

IMAGES, DISTINCT, WARMUP, ROUNDS, CALLS = 2048, 8, 3, 7, 20
SIZES = ((64, 16), (128, 32))


def spread(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "samples": len(ts)}


def stroke_image(size, seed):
    rng = np.random.default_rng(seed)
    a = np.full((size, size), 255, np.uint8)
    for _ in range(5):
        x, y = rng.integers(8, size - 8), rng.integers(8, size - 8)
        for _ in range(size):
            x, y = int(np.clip(x + rng.integers(-2, 3), 2, size - 3)), int(np.clip(y + rng.integers(-1, 2), 2, size - 3))
            a[y - 1:y + 2, x - 1:x + 2] = rng.integers(0, 90)
    return a


def weight_matrix(extent, c, dev):
    """(extent, grid) float32: row x holds B_a(x mod c) / 6 c^3 at columns x // c + a."""
    g = -(-extent // c) + 3
    m = np.zeros((extent, g), np.float64)
    x = np.arange(extent)
    b = W.weights(x % c, c) / (6.0 * c ** 3)
    for a in range(4):
        m[x, x // c + a] = b[a]
    return torch.from_numpy(m.astype(np.float32)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"device_name": torch.cuda.get_device_name(0), "images": IMAGES, "distinct_images": DISTINCT, "warmup_rounds": WARMUP,
           "rounds": ROUNDS, "calls_per_round": CALLS}

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / CALLS

    for size, c in SIZES:
        distinct = np.stack([stroke_image(size, 40 + i) for i in range(DISTINCT)])
        src = torch.from_numpy(distinct[np.arange(IMAGES) % DISTINCT]).to(dev)
        out = torch.empty_like(src)
        amp = W.max_amp(c)
        spec = warp.WarpSpec(cell=c, amplitude=amp / 256.0)
        ids = np.arange(IMAGES, dtype=np.uint64)
        rows = torch.from_numpy(warp.param_rows(np.arange(IMAGES, dtype=np.uint64), (amp, amp), np.array([W.IDENTITY] * IMAGES))).to(dev)
        gy, gx = W.grid(size, size, c)
        by, bx = weight_matrix(size, c, dev), weight_matrix(size, c, dev)
        base = torch.stack(torch.meshgrid(torch.arange(size, device=dev, dtype=torch.float32),
                                          torch.arange(size, device=dev, dtype=torch.float32), indexing="ij")[::-1], -1)   # (h, w, 2): x, y
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)

        def hip_call():
            warp.warp_u8(src, spec, 5, draw_ids=ids, out=out)

        def hip_resident():
            _lib.check(lib.siggan_warp_u8(0, _call.ptr(src), IMAGES, None, _call.ptr(rows), None, _call.ptr(out), None, IMAGES, size, size, c,
                                          255, 5, _call.stream(dev)))

        def torch_call():
            d = (torch.rand((IMAGES, 2, gy, gx), device=dev, generator=gen) * 2 - 1) * (amp / 256.0)
            disp = by @ d @ bx.t()                                                    # (n, 2, h, w)
            grid = (base + disp.permute(0, 2, 3, 1)) * (2.0 / (size - 1)) - 1.0
            img = F.grid_sample(src[:, None].float() - 255.0, grid, mode="bilinear", padding_mode="zeros", align_corners=True) + 255.0
            return img.round_().clamp_(0, 255).to(torch.uint8)

        entry = {}
        # alternate the three so that a drift of the machine falls on all of them
        samples = {"hip": [], "hip_resident_rows": [], "torch": []}
        for name, fn in (("hip", hip_call), ("hip_resident_rows", hip_resident), ("torch", torch_call)):
            for _ in range(WARMUP):
                events(fn)
        for _ in range(ROUNDS):
            for name, fn in (("hip", hip_call), ("hip_resident_rows", hip_resident), ("torch", torch_call)):
                samples[name].append(events(fn))
        for name, ts in samples.items():
            entry[name] = {**spread(ts), "images_per_s": IMAGES / statistics.median(ts), "us_per_call": 1e6 * statistics.median(ts)}
        entry["torch_over_hip"] = entry["torch"]["median_s"] / entry["hip"]["median_s"]
        entry["torch_over_hip_resident_rows"] = entry["torch"]["median_s"] / entry["hip_resident_rows"]["median_s"]
        hip_resident()
        want, _ = W.warp_one(distinct[0], 5, 0, (amp, amp), W.IDENTITY, c, 255)
        entry["equals_restatement"] = bool(np.array_equal(out[0].cpu().numpy(), want))
        entry["bytes_moved_per_call"] = 2 * IMAGES * size * size
        entry["cell"], entry["amplitude_q8"] = c, amp
        res[f"{size}x{size}"] = entry
        print(size, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
