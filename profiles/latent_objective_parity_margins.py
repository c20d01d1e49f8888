"""Writes profiles/latent_objective_parity_margins.json: what tests/test_latent_objective_gpu.py and tests/test_refine_gpu.py
bound, as measured -- per case and weight set the gradient's distance from the fp64 oracle (of max|dz_ref|, bound 1e-4) and the
relative errors of the realism term (bound 2^-22), the prior term (bound latent 2^-24) and the objective (bound 2^-22), the
device's logits, the borderline decisions in both networks; for the refinement loop the gradient along the path and the
oracle's and the device's drop of the objective over the 20 steps (bound: device >= oracle / 2).  Needs the GPU.

    python profiles/latent_objective_parity_margins.py [--out profiles/latent_objective_parity_margins.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_objective_parity_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("latent_objective_parity_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import test_latent_objective_gpu as T
    import test_refine_gpu as R
    from hipcommon import count_sign_flips
    from latentcommon import P_LATENT, P_SIZE, oracle_sd64
    from objectivecommon import CASES, R_LR, R_STEPS, oracle_d_sd64, oracle_objective, oracle_refine

    out = {"gradient_bound": 1e-4, "realism_term_bound": 2.0 ** -22, "objective_bound": 2.0 ** -22, "cases": [], "loop": {}}
    for case in CASES:
        run = T.compute_case(case)
        p = run[T.ALL3][3].double()
        row = {"size": case[0], "latent": case[1], "batch": case[2], "g_leaky_slope": case[3], "spectral_norm": case[4],
               "device_logits": (torch.log(p) - torch.log1p(-p)).tolist(), "prior_term_bound": case[1] * 2.0 ** -24,
               "borderline_decisions_g": count_sign_flips(run["signs_g"], run["rec_g"]),
               "borderline_decisions_d": count_sign_flips(run["signs_d"], run["rec_d"]),
               "activations": int(sum(t.numel() for t in run["rec_g"] + run["rec_d"])), "weights": []}
        grad, term = T.grad_margins(run), T.term_margins(run)
        for w in grad:
            row["weights"].append({"recon_realism_prior": list(w), "dz_err_over_max_ref": grad[w][0], "max_abs_dz_ref": grad[w][1],
                                   "realism_rel_err": term[w][0], "prior_rel_err": term[w][1], "objective_rel_err": term[w][2]})
        out["cases"].append(row)
    run = R.compute_refinement()
    path = {}
    for k, (z_k, dz, signs_g, signs_d) in run["probes"].items():
        ref = oracle_objective(oracle_sd64(P_SIZE, P_LATENT), oracle_d_sd64(P_SIZE), z_k, None, P_SIZE, signs_g, signs_d)[1][1]
        path[str(k)] = float((dz.double() - ref).abs().max()) / float(ref.abs().max())
    ref, logits, z_ref = oracle_refine(run["z0"], R_STEPS, R_LR)
    z_ref_p = oracle_refine(run["z0"], R_STEPS, R_LR, prior_weight=0.1)[2]
    dev = run["loop"][1].double()
    rms = lambda z: float((z.double() ** 2).mean()) ** 0.5
    out["loop"] = {"steps": int(dev.shape[0]), "lr": R_LR, "dz_err_over_max_ref_at_step": path,
                   "oracle_objective_first": ref[0].tolist(), "oracle_objective_last": ref[-1].tolist(),
                   "oracle_logit_rise": (logits[-1] - logits[0]).tolist(),
                   "device_objective_first": dev[0].tolist(), "device_objective_last": dev[-1].tolist(),
                   "bound": "device drop >= oracle drop / 2, oracle drop > 0.1",
                   "probs_before": run["loop"][4].tolist(), "probs_after": run["loop"][2].tolist(),
                   "rms_z": {"device": rms(run["loop"][0]), "device_prior_0.1": rms(run["z_prior"]), "oracle": rms(z_ref),
                             "oracle_prior_0.1": rms(z_ref_p)}}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
