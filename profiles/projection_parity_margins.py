"""Writes profiles/projection_parity_margins.json: what tests/test_projection_gpu.py and tests/test_latent_grad_gpu.py bound,
as measured -- per case the gradient's distance from the fp64 oracle (of max|dz_ref|, bound 1e-4), the loss' relative distance
from numpy fp64 (bound S^2 2^-24), the borderline decisions; for the loop the oracle's and the device's loss reduction over the
40 steps (bound: device >= oracle / 2).  Needs the GPU.

    python profiles/projection_parity_margins.py [--out profiles/projection_parity_margins.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_parity_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("projection_parity_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import test_latent_grad_gpu as T
    import test_projection_gpu as P
    from hipcommon import count_sign_flips
    from latentcommon import oracle_descent

    out = {"gradient_bound": 1e-4, "cases": [], "loop": {}}
    for case in T.CASES:
        run = T.compute_case(case)
        ref = run["dz_ref"]
        x = run["img"][:, 0].double().numpy()
        want = ((x - run["t64"]) ** 2).mean(axis=(1, 2))
        out["cases"].append({
            "size": case[0], "latent": case[1], "batch": case[2], "g_leaky_slope": case[3],
            "dz_err_over_max_ref": float((run["dz"].double() - ref).abs().max()) / float(ref.abs().max()),
            "max_abs_dz_ref": float(ref.abs().max()),
            "loss": run["loss"].tolist(), "loss_rel_err": float((np.abs(run["loss"].double().numpy() - want) / want).max()),
            "loss_rel_bound": case[0] * case[0] * 2.0 ** -24,
            "borderline_decisions": count_sign_flips(run["signs"], run["rec"]),
            "activations": int(sum(t.numel() for t in run["rec"]))})
    run = P.compute_projection()
    ref = oracle_descent(run["t64"], run["z0"])
    dev = run["loop"][1].double()
    out["loop"] = {"steps": int(dev.shape[0]), "oracle_loss_first": ref[0].tolist(), "oracle_loss_last": ref[-1].tolist(),
                   "oracle_reduction": (ref[0] / ref[-1]).tolist(), "device_loss_first": dev[0].tolist(),
                   "device_loss_last": dev[-1].tolist(), "device_reduction": (dev[0] / dev[-1]).tolist(),
                   "bound": "device_reduction >= oracle_reduction / 2"}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
