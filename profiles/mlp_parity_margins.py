"""Observed parity margins of the fully-connected GAN's HIP steps on the MI355X: every bounded comparison of
tests/test_mlp_steps_gpu.py (HIP against the fp64 oracle run from HIP's own state before the step: metrics, every gradient
tensor, the BatchNorm running statistics; chained, clipped and batch-1 steps) with its relative deviation and its bound.

    python profiles/mlp_parity_margins.py --out profiles/mlp_parity_margins.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import torch                                                          # noqa: E402

import mlpcommon as MC                                                # noqa: E402
import test_mlp_steps_gpu as T                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_parity_margins.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    T.MARGINS = {}
    for case in MC.CASES:
        T.test_chained_steps(case)
    for factor in (0.5, 2.0):
        T.test_clipping(factor)
    T.test_batch_one()
    ratio = lambda v: v["deviation"] / v["bound"] if v["bound"] > 0 else float("inf")      # noqa: E731
    worst = max(T.MARGINS.items(), key=lambda kv: ratio(kv[1]))
    out = {"device": torch.cuda.get_device_name(0),
           "rule": "relative deviation per tensor <= min(32 x fp32-oracle-vs-fp64-oracle deviation, 1e-4); a metric's deviation estimate is floored at 2^-24",
           "cases": {c.name: c._asdict() for c in MC.CASES + (MC.ONE,)}, "comparisons": len(T.MARGINS),
           "closest_to_its_bound": {worst[0]: dict(worst[1], ratio=ratio(worst[1]))}, "margins": T.MARGINS}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("device", "comparisons", "closest_to_its_bound")}, indent=1))


if __name__ == "__main__":
    main()
