"""Throughput of the latent objective on the MI355X, 64x64, latent 100.

    python profiles/latent_objective_throughput.py [--out profiles/latent_objective_throughput.json] [--only-latent-grad]

Per call at batch 64: Engine.g_latent_objective_grad with the weights (1,0,0), (0,1,0) and (1,1,0.1), and Engine.g_latent_grad
beside them.  Method (as profiles/projection_throughput.py): the reference's init distribution (seeded), targets = the bytes of G
at seeded z; WARMUP calls, then REPEATS windows of ITERS calls per variant, every window timed by a host clock around enqueue +
torch.cuda.synchronize() and by a pair of device events, the variants alternating window by window so that a drift of the shared
host hits all alike.  Reported per variant: the median window's ms per call, min / max over the windows.

``--only-latent-grad`` measures g_latent_grad alone, which also runs on a commit that does not have the objective yet: run on
the parent commit it gives the parent's figure, and its repeats (SESSIONS fresh contexts of REPEATS windows each) the
parent's own run-to-run spread.

End to end: refine_latents on n = 1000 for 20 steps beside generate_signatures_filtered keeping 1000 of 2000, batch 64, both
from modules on one engine, one warm run then the median of three.  Needs the GPU: there is no CPU path and no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd.engine import Engine  # noqa: E402

SIZE, LATENT, BATCH = 64, 100, 64
WARMUP, ITERS, REPEATS, SESSIONS = 20, 1000, 7, 3
VARIANTS = {"objective_1_0_0": (1.0, 0.0, 0.0), "objective_0_1_0": (0.0, 1.0, 0.0), "objective_1_1_0.1": (1.0, 1.0, 0.1)}


class Calls:
    def __init__(self):
        self.eng = Engine(latent_dim=LATENT, image_size=SIZE, max_batch=BATCH, device="cuda:0", seed=1)
        self.eng.init_reference(seed=0)
        gen = torch.Generator().manual_seed(BATCH)
        self.t = self.eng.g_generate_u8(torch.randn(BATCH, LATENT, generator=gen).cuda())
        self.z = torch.randn(BATCH, LATENT, generator=gen).cuda()
        self.dz, self.obj = torch.empty_like(self.z), torch.empty(BATCH, device="cuda:0")

    def call(self, name):
        if name == "g_latent_grad":
            self.eng.g_latent_grad(self.z, self.t, dz_out=self.dz, loss_out=self.obj)
        else:
            w = VARIANTS[name]
            self.eng.g_latent_objective_grad(self.z, self.t if w[0] else None, *w, dz_out=self.dz, objective_out=self.obj)

    def window(self, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(ITERS):
            self.call(name)
        e1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3


def measure(names):
    c = Calls()
    for n in names:
        for _ in range(WARMUP):
            c.call(n)
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(REPEATS):
        for n in names:
            times[n].append(c.window(n))
    c.eng.close()
    out = {}
    for n in names:
        host, dev = sorted(t for t, _ in times[n]), sorted(t for _, t in times[n])
        out[n] = {"ms_per_call_median": 1e3 * statistics.median(host) / ITERS, "ms_per_call_min": 1e3 * host[0] / ITERS,
                  "ms_per_call_max": 1e3 * host[-1] / ITERS, "ms_per_call_device_events_median": 1e3 * statistics.median(dev) / ITERS}
    return out


def end_to_end():
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    from signature_gan_amd.utils.inference import generate_signatures_filtered, refine_latents
    eng = Engine(latent_dim=LATENT, image_size=SIZE, max_batch=BATCH, device="cuda:0", seed=1)
    g, d = Generator(latent_dim=LATENT, output_size=SIZE, _engine=eng).eval(), Discriminator(input_size=SIZE, _engine=eng).eval()
    eng.init_reference(seed=0)
    z0 = torch.randn(1000, LATENT, generator=torch.Generator().manual_seed(3))

    def timed(fn):
        fn()
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return {"seconds_median": statistics.median(ts), "seconds_min": min(ts), "seconds_max": max(ts)}

    out = {"refine_latents_n1000_steps20": timed(lambda: refine_latents(g, d, z0, steps=20, lr=0.02)),
           "generate_signatures_filtered_keep1000_of_2000": timed(lambda: generate_signatures_filtered(
               g, d, 1000, LATENT, torch.device("cuda:0"), seed=3, batch_size=BATCH, oversampling_ratio=2.0))}
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_objective_throughput.json"))
    ap.add_argument("--only-latent-grad", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_objective_throughput.py measures on the MI355X: no ROCm device found")
    out = {"device": torch.cuda.get_device_name(0), "size": SIZE, "latent": LATENT, "batch": BATCH, "calls_per_window": ITERS,
           "windows": REPEATS, "warmup_calls": WARMUP, "clock": "host perf_counter around enqueue + synchronize; device events beside it"}
    out["g_latent_grad_sessions"] = [measure(["g_latent_grad"])["g_latent_grad"] for _ in range(SESSIONS)]
    if not a.only_latent_grad:
        out["per_call"] = measure(["g_latent_grad"] + list(VARIANTS))
        out["end_to_end"] = end_to_end()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
