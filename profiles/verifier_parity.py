"""Worst deviation of the HIP signature verifier from the reference's fp64 result, per tensor and fixture case, next to
the bound the tests hold it to (tests/verifiercommon.py).  Run on the MI355X:

    python profiles/verifier_parity.py --out profiles/verifier_parity_margins.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import torch                                                          # noqa: E402

import verifiercommon as VC                                           # noqa: E402
from verifiercommon import VI                                         # noqa: E402
from test_verifier_gpu import DEV, cuda, make_ctx                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verifier_parity_margins.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "bound": "min(32 x reference fp32-vs-fp64 deviation, 1e-4); probes relative "
           "to the tensor's max-abs (listed absolute), embeddings and scores absolute", "cases": {}}
    for n_pairs, e in VI.CASES:
        f = VC.load_case(n_pairs, e)
        x1, x2, _ = VC.case_inputs(n_pairs)
        ctx = make_ctx(e, 2 * n_pairs)
        e1, e2, s = ctx.score(cuda(x1), cuda(x2))
        m = {}
        for name, shape in VI.STAGES:
            got = VC.probe(ctx.debug_tensor(name, (2 * n_pairs,) + shape).cpu(), name)
            m[name] = {"deviation": VC.deviation(got, f, name), "bound": VC.bound(f, name)}
        for name, t in (("e1", e1), ("e2", e2), ("similarity", s)):
            m[name] = {"deviation": VC.deviation(t.cpu().numpy(), f, name), "bound": VC.bound(f, name)}
        for v in m.values():
            v["fraction_of_bound"] = v["deviation"] / v["bound"]
        out["cases"][f"pairs={n_pairs},E={e}"] = m
        ctx.close()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
