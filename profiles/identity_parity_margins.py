"""Writes profiles/identity_parity_margins.json: what tests/test_verifier_input_grad_gpu.py and tests/test_latent_seed_gpu.py
bound, as measured -- per verifier case the input gradient's and the terms' distance from the fp64 restatement on the device's
own decisions (of max|dx_ref| / max|term_ref|, bound 1e-4), the device's logits' range, the dead share of every pooling layer
and the decisions that differ from the fp64 run's own (all of them borderline, or the test fails); per seeded Generator case the
seed-only dz's distance from the oracle's J^T seed and that of the seed's share of a full (1, 1, 1) objective (bound 1e-4 of
max|J^T seed|).  Needs the GPU.

    python profiles/identity_parity_margins.py [--out profiles/identity_parity_margins.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_parity_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("identity_parity_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import identitycommon as IC
    import test_latent_seed_gpu as S
    import test_verifier_input_grad_gpu as V

    out = {"bound": IC.BOUND, "near_tie": IC.NEAR_TIE, "verifier_input_grad": [], "seeded_latent_grad": []}
    for case in V.CASES:
        run = V.compute_case(case)
        err, scale, terr = V.grad_margins(run)
        diff = IC.differing(run["dec"], run["own"]["decisions"], run["margins"])
        out["verifier_input_grad"].append({
            "n_images": case[0], "embedding_dim": case[1], "embed_score_weights": list(case[2]), "dx_err_over_max_ref": err,
            "max_abs_dx_ref": scale, "terms_err_over_max_ref": terr, "max_abs_logit": float(run["ref"]["logit"].abs().max()),
            "dead_share": IC.dead_fraction(run["dec"]),
            "decisions_differing_from_fp64": {k: {"differing": d, "of_those_borderline": n} for k, (d, n) in diff.items()}})
    for case in S.CASES64:
        run = S.compute_case(case)
        ref = run["dz_ref"]
        scale = float(ref.abs().max())
        share = run["seeded", S.ONES][0].double() - run["plain", S.ONES][0].double()
        out["seeded_latent_grad"].append({
            "size": case[0], "latent": case[1], "batch": case[2], "g_leaky_slope": case[3], "spectral_norm": case[4],
            "max_abs_dz_ref": scale, "seed_only_dz_err_over_max_ref": float((run["seed1"][0].double() - ref).abs().max()) / scale,
            "seed_share_of_111_err_over_max_ref": float((share - ref).abs().max()) / scale,
            "max_abs_dz_unseeded_111": float(run["plain", S.ONES][0].abs().max())})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
