"""Throughput of the parameter gradient and of one adaptation iteration on the MI355X, 64x64, latent 100.

    python profiles/adapt_throughput.py [--out profiles/adapt_throughput.json]

Per batch (8 and 64), measured in ONE session with the variants alternating window by window (a drift of the shared host hits
all alike):
  g_param_grad_fl0 / _fl3 / _fl5      Engine.g_param_grad with the weights (1, 0) and first_layer 0, 3, Lg + 1
  g_param_grad_fl0_realism            ... first_layer 0 with the weights (1, 1): the Discriminator's forward and input-gradient chain too
  g_param_grad_fl0_repacked           ... first_layer 0 with Engine.params_changed() in front of every call: the difference to
                                      g_param_grad_fl0 is what re-packing both networks costs an iteration
  adapt_iteration_fl0 / _fl3          g_param_grad + op_adam on the trainable suffix + params_changed: adapt_generator's loop body
  g_latent_grad                       the latent gradient at the same batch
  g_step                              one Generator training step (forward, Discriminator pass, backward, update)
Method (as profiles/latent_objective_throughput.py): the reference's init distribution (seeded), targets = the bytes of G at
seeded z; WARMUP calls, then REPEATS windows of ITERS calls per variant, every window timed by a host clock around enqueue +
torch.cuda.synchronize() and by a pair of device events.  Reported per variant: the median window's ms per call, min / max over
the windows.  The adaptation variants run with lr = 0, so the weights stay where they are.  Needs the GPU: there is no CPU path."""
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

SIZE, LATENT, BATCHES = 64, 100, (8, 64)
WARMUP, ITERS, REPEATS = 20, 300, 7


class Calls:
    def __init__(self, batch):
        self.b = batch
        self.eng = eng = Engine(latent_dim=LATENT, image_size=SIZE, max_batch=batch, device="cuda:0", seed=1)
        eng.init_reference(seed=0)
        gen = torch.Generator().manual_seed(batch)
        self.t = eng.g_generate_u8(torch.randn(batch, LATENT, generator=gen).cuda())
        self.z = torch.randn(batch, LATENT, generator=gen).cuda()
        self.dz, self.obj = torch.empty_like(self.z), torch.empty(batch, device="cuda:0")
        self.d = torch.empty_like(eng.g_params)
        self.mv = {fl: (torch.zeros(eng.layer_span(fl)[1], device="cuda:0"), torch.zeros(eng.layer_span(fl)[1], device="cuda:0")) for fl in (0, 3)}
        self.k = 0

    def grad(self, fl, wd=0.0):
        self.eng.g_param_grad(self.z, self.t, 1.0, wd, first_layer=fl, dparams_out=self.d, objective_out=self.obj)

    def call(self, name):
        eng = self.eng
        if name == "g_latent_grad":
            eng.g_latent_grad(self.z, self.t, dz_out=self.dz, loss_out=self.obj)
        elif name == "g_step":
            eng.g_step(self.b, self.z, lr=0.0, sync=False)
        elif name == "g_param_grad_fl0_realism":
            self.grad(0, 1.0)
        elif name == "g_param_grad_fl0_repacked":
            eng.params_changed()
            self.grad(0)
        elif name.startswith("g_param_grad_fl"):
            self.grad(int(name[len("g_param_grad_fl"):]))
        else:
            fl = int(name[len("adapt_iteration_fl"):])
            off = eng.layer_span(fl)[0]
            self.grad(fl)
            self.k += 1
            eng.op_adam(eng.g_params[off:], self.d[off:], *self.mv[fl], self.k, lr=0.0, beta1=0.9, beta2=0.999, grad_scale=1.0 / self.b)
            eng.params_changed()

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


def measure(batch):
    c = Calls(batch)
    lg = c.eng.g_layers
    names = [f"g_param_grad_fl{fl}" for fl in (0, 3, lg + 1)] + ["g_param_grad_fl0_realism", "g_param_grad_fl0_repacked",
                                                                  "adapt_iteration_fl0", "adapt_iteration_fl3", "g_latent_grad", "g_step"]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_throughput.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adapt_throughput.py measures on the MI355X: no ROCm device found")
    out = {"device": torch.cuda.get_device_name(0), "size": SIZE, "latent": LATENT, "calls_per_window": ITERS, "windows": REPEATS,
           "warmup_calls": WARMUP, "clock": "host perf_counter around enqueue + synchronize; device events beside it",
           "batch": {str(b): measure(b) for b in BATCHES}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
