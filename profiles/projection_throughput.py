"""Projection throughput on the MI355X: iterations per second of the loop utils.inference.project_signatures runs
(Engine.g_latent_grad + Engine.op_adam on z), 64x64, latent 100, batch 64 and 256.

    python profiles/projection_throughput.py [--out profiles/projection_throughput.json]

Method: the Generator holds the reference's init distribution (seeded), the targets are the bytes of G at seeded z, the loop
starts at other seeded z.  Per batch: WARMUP iterations (code objects, the weight packs), then REPEATS windows of ITERS
iterations each, every window timed by a host clock around enqueue + torch.cuda.synchronize() and, beside it, by a pair of
device events; the windows alternate between the two batches so that a drift of the shared host hits both alike.  Reported per
batch: the median window's iterations per second and images x iterations per second, the spread (min / max over windows), the
launches per iteration (2 Lg + 7 = 15 plus the split-K tails launch_gconv adds, counted from the library's own launch
profile), and the algorithmic FLOPs of one iteration (forward + input-gradient GEMMs, fc both ways) with the rate they give --
an end-to-end figure of the loop, not a kernel's share of peak.  Needs the GPU: there is no CPU path and no fallback."""
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

SIZE, LATENT, BATCHES = 64, 100, (64, 256)
WARMUP, ITERS, REPEATS = 20, 200, 7
G_CHAIN = (256, 128, 64, 32, 32)


def iteration_flops(batch):
    """2 x MACs of one iteration: fc forward and dz, every transposed-conv block forward and its input-gradient, the final
    3x3 conv forward and its input-gradient (padding taps included, as the GEMMs compute them)."""
    f = 2.0 * batch * (G_CHAIN[0] * 16) * LATENT * 2
    for l in range(1, len(G_CHAIN)):
        hi = 4 << (l - 1)
        f += 2.0 * batch * hi * hi * G_CHAIN[l - 1] * G_CHAIN[l] * 16 * 2
    f += 2.0 * batch * SIZE * SIZE * G_CHAIN[-1] * 9 * 2
    return f


class Loop:
    def __init__(self, batch):
        self.batch = batch
        self.eng = Engine(latent_dim=LATENT, image_size=SIZE, max_batch=batch, device="cuda:0", seed=1)
        self.eng.init_reference(seed=0)
        gen = torch.Generator().manual_seed(batch)
        self.t = self.eng.g_generate_u8(torch.randn(batch, LATENT, generator=gen).cuda())
        self.z = torch.randn(batch, LATENT, generator=gen).cuda()
        self.m, self.v, self.dz = torch.zeros_like(self.z), torch.zeros_like(self.z), torch.empty_like(self.z)
        self.loss = torch.empty(batch, device="cuda:0")
        self.k = 0

    def run(self, n):
        for _ in range(n):
            self.k += 1
            self.eng.g_latent_grad(self.z, self.t, dz_out=self.dz, loss_out=self.loss)
            self.eng.op_adam(self.z, self.dz, self.m, self.v, self.k, lr=0.05, beta1=0.9, beta2=0.999)

    def window(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        self.run(ITERS)
        e1.record()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3

    def launches(self):
        """implicit-GEMM launches of one g_latent_grad as the library's profile lists them (split-K tails are not in it)."""
        self.eng.prof_enable(True)
        self.eng.g_latent_grad(self.z, self.t, dz_out=self.dz, loss_out=self.loss)
        torch.cuda.synchronize()
        rows = self.eng.prof_launches()
        self.eng.prof_enable(False)
        return [{k: r[k] for k in ("kernel", "form", "epi", "M", "Ci", "Co")} for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_throughput.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("projection_throughput.py measures on the MI355X: no ROCm device found")
    loops = {b: Loop(b) for b in BATCHES}
    for lp in loops.values():
        lp.run(WARMUP)
    torch.cuda.synchronize()
    times = {b: [] for b in BATCHES}
    for _ in range(REPEATS):
        for b in BATCHES:                                    # alternate the batches window by window
            times[b].append(loops[b].window())
    out = {"device": torch.cuda.get_device_name(0), "size": SIZE, "latent": LATENT, "iters_per_window": ITERS, "windows": REPEATS,
           "warmup_iters": WARMUP, "clock": "host perf_counter around enqueue + synchronize; device events beside it", "batches": {}}
    for b in BATCHES:
        host = sorted(t for t, _ in times[b])
        dev = sorted(t for _, t in times[b])
        med = statistics.median(host)
        out["batches"][str(b)] = {
            "iters_per_s_median": ITERS / med, "iters_per_s_min": ITERS / host[-1], "iters_per_s_max": ITERS / host[0],
            "image_iters_per_s_median": b * ITERS / med, "ms_per_iter_median": 1e3 * med / ITERS,
            "ms_per_iter_device_events_median": 1e3 * statistics.median(dev) / ITERS,
            "gflop_per_iter": iteration_flops(b) * 1e-9, "end_to_end_tflops_median": iteration_flops(b) * ITERS / med * 1e-12,
            "final_loss_mean": float(loops[b].loss.mean()), "gemm_launches": loops[b].launches()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({b: {k: v for k, v in r.items() if k != "gemm_launches"} for b, r in out["batches"].items()}, indent=1))


if __name__ == "__main__":
    main()
