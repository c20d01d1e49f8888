#!/usr/bin/env python3
"""Pairs per second of siggan_ssim_pairs on the MI355X, and of the same definition in numpy on the host.

    python profiles/ssim_throughput.py [--out profiles/ssim_throughput.json]

Two device cases at 64 x 64, on bytes that are already on the device and on sets that are already prepared:
  "best_1000x2640"   ssim_best of 1 000 generated against 2 640 real images (2.64 M pairs), best / index only: no matrix
  "matrix_512x512"   ssim_matrix of 512 images against themselves (SAME_SET, 262 144 entries)
and beside them "prepare" (SsimSet of the 2 640 and of the 1 000 images: what is paid once per set).  Device events around
CALLS back-to-back calls; the median with min and max of ROUNDS samples after WARMUP rounds.  The generated side is the bytes
of a reference_init Generator whose final conv is scaled by 1024 (no trained checkpoint ships with the code), the real side
blurred poly-lines, each rolled by its own offset so that no two images are equal.

"host": the float64 restatement of tests/ssimcommon.py (numpy, vectorised over the second set) and scipy's correlate1d
formulation pair by pair, on ONE thread, on HOST_A x HOST_B pairs of the same images; the device's values for those pairs are
checked against it.  No ratio is a pass condition.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssimcommon as SC  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import ssim  # noqa: E402

WARMUP, ROUNDS, CALLS, HOST_ROUNDS, HOST_A, HOST_B, SIZE = 3, 10, 3, 3, 8, 64, 64
N_GENERATED, N_REAL, N_MATRIX = 1000, 2640, 512


def generator_bytes(n, dev):
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=100, output_size=SIZE).to(dev).eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
    g._engine.params_changed()
    torch.manual_seed(11)
    parts = [g._engine.g_generate_u8(torch.randn(64, 100, device=dev)).reshape(64, SIZE, SIZE).clone() for _ in range((n + 63) // 64)]
    return torch.cat(parts)[:n].contiguous()


def real_bytes(n, dev):
    base = [SC.strokes(SIZE, SIZE, 1000 + i) for i in range(66)]
    rng = np.random.default_rng(3)
    out = [np.roll(base[i % len(base)], (int(rng.integers(0, SIZE)), int(rng.integers(0, SIZE))), axis=(0, 1)) for i in range(n)]
    return torch.from_numpy(np.stack(out)).to(dev)


def spread(ts, pairs=None):
    d = {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts), "samples": len(ts)}
    if pairs is not None:
        d["pairs"] = pairs
        d["pairs_per_second"] = pairs / statistics.median(ts)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")

    def events(fn, calls=CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / calls

    fake, real = generator_bytes(N_GENERATED, dev), real_bytes(N_REAL, dev)
    fake_set, real_set, small = ssim.SsimSet(fake), ssim.SsimSet(real), ssim.SsimSet(fake[:N_MATRIX])
    routes = {"best_1000x2640": (lambda: ssim.ssim_best(fake_set, real_set), N_GENERATED * N_REAL),
              "matrix_512x512": (lambda: ssim.ssim_matrix(small), N_MATRIX * N_MATRIX),
              "prepare": (lambda: (ssim.SsimSet(fake), ssim.SsimSet(real)), None)}
    for _ in range(WARMUP):
        for fn, _n in routes.values():
            events(fn, 1)
    times = {k: [] for k in routes}
    for _ in range(ROUNDS):
        for k, (fn, _n) in routes.items():
            times[k].append(events(fn))
    res = {"device_name": torch.cuda.get_device_name(0), "size": SIZE, "warmup_rounds": WARMUP, "calls_per_event_sample": CALLS,
           "device": {k: spread(times[k], routes[k][1]) for k in routes}}
    res["device"]["prepare"]["images"] = N_GENERATED + N_REAL

    # the host, one thread, on a subsample; and the device's values for the same pairs
    ha, hb = fake[:HOST_A].cpu().numpy(), real[:HOST_B].cpu().numpy()
    SC.ssim_matrix64(ha[:2], hb[:4])
    vec, loop, m64 = [], [], None
    for _ in range(HOST_ROUNDS):
        t0 = time.perf_counter()
        m64 = SC.ssim_matrix64(ha, hb)
        vec.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ms = np.array([[SC.ssim_scipy(x, y) for y in hb[:8]] for x in ha])
        loop.append(time.perf_counter() - t0)
    got = ssim.ssim_matrix(fake[:HOST_A].contiguous(), real[:HOST_B].contiguous()).cpu().numpy().astype(np.float64)
    best, index = ssim.ssim_best(fake_set, real_set)
    rows = ssim.ssim_matrix(fake[:HOST_A].contiguous(), real_set).cpu().numpy()
    res["host"] = {"threads": 1, "numpy_float64_vectorised": spread(vec, HOST_A * HOST_B), "scipy_pair_by_pair": spread(loop, HOST_A * 8),
                   "device_minus_float64_max": float(np.abs(got - m64).max()),
                   "scipy_minus_float64_max": float(np.abs(ms - m64[:, :8]).max()),
                   "best_equals_first_maximum_of_matrix_rows": bool(np.array_equal(index[:HOST_A].cpu().numpy(), rows.argmax(axis=1))
                                                                    and np.array_equal(best[:HOST_A].cpu().numpy(), rows.max(axis=1)))}
    host_rate = res["host"]["numpy_float64_vectorised"]["pairs_per_second"]
    res["device_over_host_pairs_per_second"] = {k: res["device"][k]["pairs_per_second"] / host_rate for k in ("best_1000x2640", "matrix_512x512")}
    res["host_seconds_for_2_64M_pairs_at_that_rate"] = N_GENERATED * N_REAL / host_rate
    print(json.dumps(res, indent=2), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
