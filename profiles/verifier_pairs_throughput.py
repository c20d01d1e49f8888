#!/usr/bin/env python3
"""Time of all-pairs scoring (siggan_verifier_pairs) on the MI355X against the only route there is without it.

    python profiles/verifier_pairs_throughput.py [--out profiles/verifier_pairs_throughput.json]

n unit-norm rows of dim 128 (what the verifier's embeddings look like), n / 16 writers, a SiameseNetwork(128) with torch's
default initialisation (seeded); one set against itself (same_set):
  "fused"            one SiameseNetwork.pairs call: counts over T = 4096 thresholds plus every row's best genuine / impostor
                     match, at n = 4096 and n = 16384.  The row maxima need every ordered pair, so all n^2 pairs are scored.
  "fused_matrix"     the same call with the (n, n) matrix written as well, n = 4096
  "fused_counts"     the counts alone: tiles on or below the diagonal are skipped, n (n - 1) / 2 pairs (plus the diagonal tiles)
  "expanded"         siggan_verifier_compare on index-expanded embeddings, the expansion included, chunked to 2^20 pairs (1 GiB of
                     expanded rows): the same n^2 pairs at n = 4096, the first n / 16 query rows (1 / 16 of the pairs) at
                     n = 16384.  It yields the scores only -- no counts, no maxima.
Device events around each call; WARMUP calls, then CALLS windows alternating between the routes; medians with min and max.
FLOP = 2 * 128 * 64 per scored pair (classifier.0 alone), against the 157.3 TFLOP/s fp32 matrix peak.  Needs the GPU; there is
no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import signature_verifier_eval as SV  # noqa: E402

DIM, HIDDEN, T = 128, 64, 4096
WARMUP, CALLS, CALLS_EXPANDED = 3, 10, 5
CHUNK_PAIRS = 1 << 20
FP32_MATRIX_PEAK_TFLOPS = 157.3
FRACTION_16384 = 16                                          # the expanded route scores 1 / 16 of the pairs at n = 16384


def unit_rows(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(n, DIM, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().to(dev).contiguous()


def spread(ts):
    return {"median_ms": 1e3 * statistics.median(ts), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "calls": len(ts)}


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def expanded(model, e, rows):
    """compare() over (e[i], e[j]) for i < rows, all j; the scores of the last chunk are returned (the rest are dropped)."""
    n = e.shape[0]
    step = max(1, CHUNK_PAIRS // n)
    cols = torch.arange(n, device=e.device)
    s = None
    for lo in range(0, rows, step):
        hi = min(lo + step, rows)
        qi = torch.arange(lo, hi, device=e.device).repeat_interleave(n)
        s = model.compare(e[qi], e[cols.repeat(hi - lo)])
    return s, lo, hi


def rate(pairs, seconds):
    tf = pairs * 2.0 * DIM * HIDDEN / seconds * 1e-12
    return {"pairs_per_s": pairs / seconds, "tflops": tf, "fraction_of_fp32_matrix_peak": tf / FP32_MATRIX_PEAK_TFLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_pairs_throughput.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    model = SV.SiameseNetwork(DIM, max_images=4).to(dev).eval()
    thr = np.unique(np.linspace(0.0, 1.0, T).astype(np.float32))
    assert thr.size == T
    out = {"device_name": torch.cuda.get_device_name(0), "dim": DIM, "thresholds": T, "warmup": WARMUP,
           "flop_per_pair": 2 * DIM * HIDDEN, "expanded_chunk_pairs": CHUNK_PAIRS, "sizes": {}}
    for n in (4096, 16384):
        e = unit_rows(n, n, dev)
        ids = (torch.arange(n, device=dev) // 16).to(torch.int32)
        rows = n if n == 4096 else n // FRACTION_16384
        routes = {"fused": (lambda: model.pairs(e, ids, e, ids, same_set=True, thresholds=thr, want_best=True), CALLS),
                  "fused_counts": (lambda: model.pairs(e, ids, e, ids, same_set=True, thresholds=thr), CALLS),
                  "expanded": (lambda: expanded(model, e, rows), CALLS_EXPANDED)}
        if n == 4096:
            routes["fused_matrix"] = (lambda: model.pairs(e, ids, e, ids, same_set=True, want_matrix=True, thresholds=thr, want_best=True), CALLS)
        last, times = {}, {name: [] for name in routes}
        for name, (fn, _) in routes.items():
            for _ in range(WARMUP if name != "expanded" else 1):
                last[name] = events(fn)[1]
        for c in range(CALLS):
            for name, (fn, calls) in routes.items():
                if c < calls:
                    times[name].append(events(fn)[0])
        res = {"n": n, "ordered_pairs": n * n, "unordered_pairs": n * (n - 1) // 2}
        for name in routes:
            med = statistics.median(times[name])
            pairs = {"fused": n * n, "fused_matrix": n * n, "fused_counts": n * (n - 1) // 2, "expanded": rows * n}[name]
            res[name] = {**spread(times[name]), "pairs_scored": pairs, **rate(pairs, med)}
        res["expanded"]["fraction_of_the_pairs"] = rows / n
        exp_full = statistics.median(times["expanded"]) * (n / rows)
        res["expanded_time_for_all_ordered_pairs_ms"] = 1e3 * exp_full
        res["fused_over_expanded_speedup"] = exp_full / statistics.median(times["fused"])
        f = last["fused"]
        res["counted_pairs"] = int(f["genuine_counts"].sum() + f["impostor_counts"].sum())
        res["counts_alone_equal_the_fused_counts"] = bool(torch.equal(last["fused_counts"]["genuine_counts"], f["genuine_counts"])
                                                          and torch.equal(last["fused_counts"]["impostor_counts"], f["impostor_counts"]))
        if n == 4096:
            s, lo, hi = last["expanded"]
            res["matrix_bit_equal_to_compare_on_the_last_chunk"] = bool(
                torch.equal(last["fused_matrix"]["score"][lo:hi].contiguous().view(torch.int32), s.view(hi - lo, n).view(torch.int32)))
        out["sizes"][str(n)] = res
        del e, last
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
