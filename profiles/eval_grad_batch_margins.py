"""Writes profiles/eval_grad_batch_margins.json: what tests/test_eval_grad_batches_gpu.py bounds, as measured -- per case of
objectivecommon.BATCH_CASES and per call (the three weight sets, g_latent_grad, the seeded call) the gradient's distance from the
fp64 oracle batch-wide (of max|dz_ref|, bound 1e-4) and on the worst row (of that row's own max|dz_ref|, bound 1e-4) with its
row index, torch fp32's per-row deviation on the same decisions and targets, the spread of the rows' gradient scales, the
borderline decisions in both networks, the largest |logit| and the seconds the oracles took; and for siggan_g_param_grad's two
batch cases every tensor's margin as profiles/param_grad_parity_margins.py records it.  Needs the GPU.

    python profiles/eval_grad_batch_margins.py [--out profiles/eval_grad_batch_margins.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_grad_batch_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("eval_grad_batch_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import evalpaths
    import test_eval_grad_batches_gpu as T
    import test_param_grad_gpu as P
    from hipcommon import count_sign_flips
    from objectivecommon import BATCH_CASES

    out = {"gradient_bound": T.BOUND, "per_row_bound": T.BOUND, "ill_conditioned_above_torch_f32": T.ILL, "cases": [], "param_grad": []}
    for case, z_seed in BATCH_CASES:
        run = T.compute_case(case, z_seed)
        p = run[T.ALL3][3].double()
        row = {"size": case[0], "latent": case[1], "batch": case[2], "g_leaky_slope": case[3], "z_seed": z_seed,
               "max_abs_logit_device": float((torch.log(p) - torch.log1p(-p)).abs().max()),
               "max_abs_logit_oracle": float(run["logit_ref"].abs().max()),
               "borderline_decisions_g": count_sign_flips(run["signs_g"], run["rec_g"]),
               "borderline_decisions_d": count_sign_flips(run["signs_d"], run["rec_d"]),
               "activations": int(sum(t.numel() for t in run["rec_g"] + run["rec_d"])), "seconds": run["seconds"],
               "paths": evalpaths.describe(*case[:3]), "calls": []}
        for call, m in T.row_margins(run).items():
            row["calls"].append({"call": list(call) if isinstance(call, tuple) else call, "dz_err_over_max_ref": m["batch"],
                                 "worst_row_err_over_row_max_ref": m["row"], "worst_row": m["at"],
                                 "torch_f32_on_that_row": m["torch_f32"], "torch_f32_worst_row": m["torch_f32_worst"],
                                 "row_scale_spread": m["scale_spread"], "smallest_row_max_abs_dz_ref": m["min_scale"]})
        out["cases"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "paths"}, indent=1))
    for case in P.PARAM_BATCH_CASES:
        run = P.compute_case(case)
        row = {"size": case[0], "latent": case[1], "batch": case[2],
               "borderline_decisions_g": count_sign_flips(run["signs_g"], run["rec_g"]),
               "borderline_decisions_d": count_sign_flips(run["signs_d"], run["rec_d"]), "weights": []}
        for w, m in P.margins(run).items():
            worst = max(m, key=lambda k: m[k][0])
            row["weights"].append({"recon_realism": list(w), "worst_tensor": worst, "worst_err_over_max_ref": m[worst][0],
                                   "smallest_max_abs_ref": min(s for _, s in m.values()),
                                   "tensors": {k: {"err_over_max_ref": e, "max_abs_ref": s} for k, (e, s) in m.items()}})
        out["param_grad"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "weights"} | {"worst": [x["worst_err_over_max_ref"] for x in row["weights"]]}))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
