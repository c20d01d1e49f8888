"""Writes profiles/param_grad_parity_margins.json: what tests/test_param_grad_gpu.py and tests/test_adapt_gpu.py bound, as
measured -- per case and weight pair every parameter tensor's distance from the fp64 oracle on the device's own decisions (of the
tensor's max|ref|, bound 1e-4) with that max|ref|, the borderline decisions in both networks, the image difference against
g_forward; the gamma-edge case; for the adaptation loop the oracle's and the device's mean loss at the start of the first and of
the last iteration (bound: device drop >= oracle drop / 2, oracle ratio < 0.5).  Needs the GPU.

    python profiles/param_grad_parity_margins.py [--out profiles/param_grad_parity_margins.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "param_grad_parity_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("param_grad_parity_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import test_adapt_gpu as A
    import test_param_grad_gpu as T
    from adaptcommon import A_LR, A_STEPS, BOUND, PARAM_WEIGHTS, oracle_adapt
    from hipcommon import count_sign_flips
    from objectivecommon import CASES

    def row_of(run):
        case = run["case"]
        row = {"size": case[0], "latent": case[1], "batch": case[2], "g_leaky_slope": case[3], "spectral_norm": case[4],
               "borderline_decisions_g": count_sign_flips(run["signs_g"], run["rec_g"]),
               "borderline_decisions_d": count_sign_flips(run["signs_d"], run["rec_d"]) if run["signs_d"] is not None else None,
               "activations": int(sum(t.numel() for t in run["rec_g"] + run["rec_d"])), "weights": []}
        for w, m in T.margins(run).items():
            worst = max(m, key=lambda k: m[k][0])
            row["weights"].append({"recon_realism": list(w), "worst_tensor": worst, "worst_err_over_max_ref": m[worst][0],
                                   "smallest_max_abs_ref": min(s for _, s in m.values()),
                                   "images_max_abs_diff_vs_g_forward": float((run[w]["images"] - run["want_img"]).abs().max()),
                                   "tensors": {k: {"err_over_max_ref": e, "max_abs_ref": s} for k, (e, s) in m.items()}})
        return row

    out = {"gradient_bound_per_tensor": BOUND, "cases": [row_of(T.compute_case(c)) for c in CASES]}
    out["gamma_edge"] = row_of(T.compute_case(CASES[0], edge=True, weights=[PARAM_WEIGHTS[0], PARAM_WEIGHTS[2]]))
    out["gamma_edge"]["entries"] = {k: dict(e) for k, e in T.EDGE.items()}
    run = A.compute_adaptation()
    loop = {"steps": A_STEPS, "lr": A_LR, "bound": "device drop >= oracle drop / 2, oracle last / first < 0.5", "first_layer": {}}
    for fl in A.FIRST:
        ref, dev = oracle_adapt(run["z0"], run["t64"], fl), run[fl]["history"].double()
        loop["first_layer"][str(fl)] = {"oracle_mean_loss_first": float(ref[0].mean()), "oracle_mean_loss_last": float(ref[-1].mean()),
                                        "device_mean_loss_first": float(dev[0].mean()), "device_mean_loss_last": float(dev[-1].mean()),
                                        "device_mean_loss_after": float(run[fl]["after"].mean())}
    loop["theta_distance_anchor_0"] = run[("anchor", 0.0)]
    loop["theta_distance_anchor_10"] = run[("anchor", 10.0)]
    out["loop"] = loop
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "cases"}, indent=1))


if __name__ == "__main__":
    main()
