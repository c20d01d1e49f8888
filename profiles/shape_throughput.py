#!/usr/bin/env python3
"""Time of the shape-attribute calls on the MI355X, and of one edit_latents iteration beside one refine_latents iteration.

    python profiles/shape_throughput.py [--out profiles/shape_throughput.json]

Per (B, s) in B = 64, 1024 and s = 64, 128, on data already on the device:
  "features"   siggan_shape_f32 with the features only (shape.shape_features)
  "grad"       siggan_shape_f32 with dx, objective and features (the loop's own call, weights validated once)
  "u8"         siggan_shape_u8 (shape.shape_sums_u8)
WARMUP calls of every route, then ROUNDS samples per route, the routes alternating.  A sample is device events around CALLS
back-to-back calls, divided by their number.  Medians with min and max, and the bytes each call must move (the image once in,
dx once out) over the median as "gb_per_s": an achieved rate of that call, launch overhead included -- not a kernel time.

"loop": a 64x64 Generator and Discriminator with the reference's initialisation on one engine, B = 64.  One iteration of
edit_latents (g_forward, shape_grad, the seeded latent call with the keep term, the add, op_adam) beside one iteration of
refine_latents (the unseeded latent call with the realism term, op_adam), the nearest existing loop.  Each is timed as a whole
call of LOOP_STEPS steps between device events, the routes alternating; the per-iteration figure is the call's time over
LOOP_STEPS, so it includes the call's set-up and end (the start features and bytes; the final evaluation; generate_uint8's
copy to the host).  There is no pass / fail threshold.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import shape as S  # noqa: E402

WARMUP, ROUNDS = 3, 9
CALLS = {64: 20000, 1024: 4000}                # back-to-back calls per sample: a tenth of a second or more
SHAPES = [(64, 64), (64, 128), (1024, 64), (1024, 128)]
LOOP_BATCH, LOOP_STEPS, LOOP_ROUNDS = 64, 50, 7


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


def kernels(dev):
    out = {}
    for b, s in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(b + s)
        x = torch.rand(b, 1, s, s, device=dev, generator=gen) * 2 - 1
        u8 = torch.randint(0, 256, (b, s, s), device=dev, generator=gen, dtype=torch.uint8)
        f0 = S.shape_features(x)
        w = torch.ones(b, 8, dtype=torch.float64, device=dev)
        t = (f0 * 1.1).contiguous()
        dx = torch.empty_like(x)
        obj = torch.empty(b, device=dev)
        routes = {"features": lambda: S.shape_features(x), "grad": lambda: S._shape_grad_checked(x, b, s, dev, w, t, dx, obj),
                  "u8": lambda: S.shape_sums_u8(u8)}
        moved = {"features": 4 * x.numel(), "grad": 8 * x.numel(), "u8": u8.numel()}
        for _ in range(WARMUP):
            for fn in routes.values():
                events(fn, 10)
        times = {k: [] for k in routes}
        for _ in range(ROUNDS):
            for k, fn in routes.items():
                times[k].append(events(fn, CALLS[b]))
        row = {k: {**spread(v), "bytes_per_call": moved[k], "gb_per_s": moved[k] / (statistics.median(v) * 1e-3) / 1e9}
               for k, v in times.items()}
        row["calls_per_sample"] = CALLS[b]
        out[f"b{b}_s{s}"] = row
        print(b, s, json.dumps(row), flush=True)
    return out


def loop(dev):
    from signature_gan_amd.engine import Engine
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    from signature_gan_amd.utils.inference import edit_latents, refine_latents
    eng = Engine(latent_dim=100, image_size=64, max_batch=LOOP_BATCH, device=str(dev), seed=1)
    g, d = Generator(latent_dim=100, output_size=64, _engine=eng).eval(), Discriminator(input_size=64, _engine=eng).eval()
    eng.init_reference(seed=0)
    z0 = torch.randn(LOOP_BATCH, 100, generator=torch.Generator().manual_seed(3))
    routes = {"edit_latents": lambda: edit_latents(g, z0, slant_delta=-0.1, size_scale=1.1, steps=LOOP_STEPS),
              "refine_latents": lambda: refine_latents(g, d, z0, steps=LOOP_STEPS)}
    for fn in routes.values():
        events(fn)
    times = {k: [] for k in routes}
    for _ in range(LOOP_ROUNDS):
        for k, fn in routes.items():
            times[k].append(events(fn) / LOOP_STEPS)
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {**{k: spread(v) for k, v in times.items()}, "batch": LOOP_BATCH, "steps_per_call": LOOP_STEPS, "image_size": 64,
           "what": "ms per iteration: a whole call's device-event time over its steps",
           "edit_over_refine": med["edit_latents"] / med["refine_latents"]}
    print("loop", json.dumps(row), flush=True)
    eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device_name": torch.cuda.get_device_name(0), "warmup_calls": 10 * WARMUP, "rounds": ROUNDS, "shapes": kernels(dev),
           "loop": loop(dev)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
