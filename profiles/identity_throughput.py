"""Throughput of the verifier's input gradient and of one identity-guided projection iteration on the MI355X, 64x64, latent 100,
batch 64, embedding 128.

    python profiles/identity_throughput.py [--out profiles/identity_throughput.json]

Measured in ONE session with the variants alternating window by window (a drift of the shared host hits all alike):
  verifier_embed            SiameseNetwork.forward_one: the five forward launches
  verifier_input_grad       SiameseNetwork.input_grad with the weights (0.5, 2): 16 launches (the five with the decisions recorded,
                            head, embedding backward, the fc1 input gradient, per conv layer an un-pool and an input gradient)
  g_forward                 Engine.g_forward(training=False): what an identity iteration runs twice
  pixel_iteration           project_signatures' loop body without the identity term: g_latent_objective_grad (1, 0, 0) + op_adam --
                            the code path of the commit before this feature, unchanged by it: the reference point of every time
  identity_iteration        g_forward -> input_grad -> the seeded g_latent_objective_grad -> torch add -> op_adam
The un-pool runs as its own launch per layer (materialised dy); a loader-fused variant was not built, so there is no comparison.
Method (as profiles/adapt_throughput.py): the reference's init distribution (seeded) for the Generator, the synthetic verifier
state of the tests, targets = the bytes of G at seeded z; WARMUP calls, then REPEATS windows of ITERS calls per variant, every
window timed by a host clock around enqueue + torch.cuda.synchronize() and by a pair of device events.  Reported per variant:
the median window's ms per call, min / max over the windows.  lr = 0, so z stays where it is.  Needs the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd.engine import Engine  # noqa: E402
from signature_gan_amd.signature_verifier_eval import SiameseNetwork  # noqa: E402

SIZE, LATENT, BATCH, E = 64, 100, 64, 128
WARMUP, ITERS, REPEATS = 20, 200, 7
W_E, W_S = 0.5, 2.0
NAMES = ("verifier_embed", "verifier_input_grad", "g_forward", "pixel_iteration", "identity_iteration")
LAUNCHES_PER_INPUT_GRAD = 16


class Calls:
    def __init__(self):
        import identitycommon as IC
        b = BATCH
        self.eng = eng = Engine(latent_dim=LATENT, image_size=SIZE, max_batch=b, device="cuda:0", seed=1)
        eng.init_reference(seed=0)
        self.v = v = SiameseNetwork(E, max_images=b)
        v.load_state_dict(IC.identity_state(E, dtype=torch.float32), strict=True)
        v.cuda().eval()
        gen = torch.Generator().manual_seed(b)
        self.t = eng.g_generate_u8(torch.randn(b, LATENT, generator=gen).cuda())
        self.ref = v.embed_u8(self.t)
        self.z = torch.randn(b, LATENT, generator=gen).cuda()
        self.m, self.s = torch.zeros_like(self.z), torch.zeros_like(self.z)
        self.dz, self.obj, self.ident = torch.empty_like(self.z), torch.empty(b, device="cuda:0"), torch.empty(b, device="cuda:0")
        self.img = torch.empty(b, 1, SIZE, SIZE, device="cuda:0")
        self.dx = torch.empty_like(self.img)
        self.k = 0

    def adam(self):
        self.k += 1
        self.eng.op_adam(self.z, self.dz, self.m, self.s, self.k, lr=0.0, beta1=0.9, beta2=0.999)

    def call(self, name):
        eng, v = self.eng, self.v
        if name == "verifier_embed":
            v.forward_one(self.img)
        elif name == "verifier_input_grad":
            v.input_grad(self.img, self.ref, W_E, W_S, dx_out=self.dx, objective_out=self.ident)
        elif name == "g_forward":
            eng.g_forward(self.z, training=False, out=self.img)
        elif name == "pixel_iteration":
            eng.g_latent_objective_grad(self.z, self.t, 1.0, 0.0, 0.0, dz_out=self.dz, objective_out=self.obj)
            self.adam()
        else:
            eng.g_forward(self.z, training=False, out=self.img)
            v.input_grad(self.img, self.ref, W_E, W_S, dx_out=self.dx, objective_out=self.ident)
            eng.g_latent_objective_grad(self.z, self.t, 1.0, 0.0, 0.0, dz_out=self.dz, objective_out=self.obj, image_grad=self.dx)
            self.obj += self.ident
            self.adam()

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


def measure():
    c = Calls()
    c.call("g_forward")
    for n in NAMES:
        for _ in range(WARMUP):
            c.call(n)
    torch.cuda.synchronize()
    times = {n: [] for n in NAMES}
    for _ in range(REPEATS):
        for n in NAMES:
            times[n].append(c.window(n))
    out = {}
    for n in NAMES:
        host, dev = sorted(t for t, _ in times[n]), sorted(t for _, t in times[n])
        out[n] = {"ms_per_call_median": 1e3 * statistics.median(host) / ITERS, "ms_per_call_min": 1e3 * host[0] / ITERS,
                  "ms_per_call_max": 1e3 * host[-1] / ITERS, "ms_per_call_device_events_median": 1e3 * statistics.median(dev) / ITERS}
    med = lambda n: out[n]["ms_per_call_median"]
    out["derived"] = {"pixel_iterations_per_s": 1e3 / med("pixel_iteration"), "identity_iterations_per_s": 1e3 / med("identity_iteration"),
                      "identity_over_pixel": med("identity_iteration") / med("pixel_iteration"),
                      "redundant_g_forward_share_of_identity_iteration": med("g_forward") / med("identity_iteration"),
                      "input_grad_over_embed": med("verifier_input_grad") / med("verifier_embed")}
    c.eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_throughput.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("identity_throughput.py measures on the MI355X: no ROCm device found")
    out = {"device": torch.cuda.get_device_name(0), "size": SIZE, "latent": LATENT, "batch": BATCH, "embedding_dim": E,
           "identity_weights": [W_E, W_S], "launches_per_input_grad_call": LAUNCHES_PER_INPUT_GRAD, "un_pool": "materialised (one launch per layer); no fused loader was built",
           "calls_per_window": ITERS, "windows": REPEATS, "warmup_calls": WARMUP,
           "clock": "host perf_counter around enqueue + synchronize; device events beside it", "variants": measure()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
