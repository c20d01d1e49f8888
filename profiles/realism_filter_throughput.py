#!/usr/bin/env python3
"""Throughput of realism-filtered generation on the MI355X: selected signatures per second.

    python profiles/realism_filter_throughput.py [--out profiles/realism_filter_throughput.json]

n = 1000 signatures kept of 2000 generated (ratio 2) in batches of 64 at 64x64, a fixed seed; reference_init networks with the
Generator's final conv and the Discriminator's classifier weight multiplied by 1024 each (fresh networks give every image the
same score, and the ranking would have only ties to rank):
  route="device"  bytes stay in an HBM pool, the Discriminator's first block reads them, one select_topk + one gather_u8
  route="host"    the pieces that existed before: bytes to the host, CPU dequantisation, fp32 upload, Discriminator.forward,
                  Python's sort
The two routes are timed alternately in windows of 20 whole runs (host clock around calls that each end in device-to-host
copies of the result, hence in a synchronise), after one warm-up of each; both return the same images and scores, which the
script checks.  Also: select_topk
alone at the cap m = 65536 (k = 32768), device events around 20 launches.  Needs the GPU; there is no fallback."""
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

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd.discriminator_vanilla_gan import Discriminator  # noqa: E402
from signature_gan_amd.engine import Engine  # noqa: E402
from signature_gan_amd.generator_vanilla_gan import Generator  # noqa: E402
from signature_gan_amd.utils.inference import generate_signatures_filtered  # noqa: E402

N, RATIO, BATCH, SIZE, LATENT, SEED, WINDOWS, RUNS = 1000, 2.0, 64, 64, 100, 5, 7, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "realism_filter_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = Generator(latent_dim=LATENT, output_size=SIZE).to(dev).eval()
    d = Discriminator(input_size=SIZE).to(dev).eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
        d.state_dict()["classifier.0.weight"].mul_(1024.0)
    g._engine.params_changed(); d._engine.params_changed()

    def run(route, runs=1):
        t0 = time.perf_counter()
        for _ in range(runs):
            images, scores = generate_signatures_filtered(g, d, N, LATENT, dev, seed=SEED, batch_size=BATCH,
                                                          oversampling_ratio=RATIO, route=route)
        return (time.perf_counter() - t0) / runs, images, scores

    ref = {}
    for route in ("device", "host"):                                    # warm-up: code objects, workspace growth, pinned buffer
        _, images, scores = run(route)
        ref[route] = (np.stack([np.array(im) for im in images]), scores)
    same = bool(np.array_equal(ref["device"][0], ref["host"][0]) and ref["device"][1] == ref["host"][1])
    times = {"device": [], "host": []}
    for _ in range(WINDOWS):
        for route in ("device", "host"):
            times[route].append(run(route, RUNS)[0])

    m, k, launches = 65536, 32768, 20
    scores = torch.rand(m, device=dev)
    Engine.select_topk(scores, k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        index = Engine.select_topk(scores, k)
    e1.record()
    torch.cuda.synchronize()
    topk_ms = e0.elapsed_time(e1) / launches
    topk_ok = bool(torch.equal(index.long(), torch.sort(scores, descending=True, stable=True).indices[:k]))

    def summary(ts):
        med = statistics.median(ts)
        return {"seconds_median": med, "seconds_min": min(ts), "seconds_max": max(ts), "selected_per_second": N / med}

    out = {"device_name": torch.cuda.get_device_name(0), "n_selected": N, "n_generated": int(N * RATIO), "batch_size": BATCH,
           "image_size": SIZE, "windows": WINDOWS, "runs_per_window": RUNS, "routes_agree": same,
           "distinct_scores_in_selection": len(set(ref["device"][1])),
           "device": summary(times["device"]), "host": summary(times["host"]),
           "speedup_median": statistics.median(times["host"]) / statistics.median(times["device"]),
           "select_topk": {"m": m, "k": k, "launches": launches, "ms_per_launch": topk_ms, "matches_stable_sort": topk_ok}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))
    assert same and topk_ok


if __name__ == "__main__":
    main()
