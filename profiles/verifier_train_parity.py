"""Observed parity margins of the HIP verifier train step on the MI355X: every comparison of tests/test_verifier_train_gpu.py's
fixture cases (HIP against the fp64 restatement given HIP's decisions, and against the fixture where no decision differs)
with its relative deviation and its bound.

    python profiles/verifier_train_parity.py --out profiles/verifier_train_parity_margins.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import torch                                                          # noqa: E402

import test_verifier_train_gpu as T                                   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_train_parity_margins.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    T.MARGINS = {}
    for v in T.VARIANTS:
        T.test_fixture_case(*v)
    worst = max(T.MARGINS.items(), key=lambda kv: kv[1]["deviation"] / kv[1]["bound"] if kv[1]["bound"] > 0 else 0.0)
    out = {"device": torch.cuda.get_device_name(0), "rule": "relative deviation per tensor <= min(32 x reference fp32-vs-fp64 deviation, 1e-4)",
           "comparisons": len(T.MARGINS), "closest_to_its_bound": {worst[0]: worst[1]}, "margins": T.MARGINS}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("device", "comparisons", "closest_to_its_bound")}, indent=1))


if __name__ == "__main__":
    main()
