"""Writes profiles/saturated_heads_margins.json: what tests/test_saturated_heads_gpu.py bounds, as measured -- per case and
dtype the worst observed FRACTION of each bound (1.0 = at the bound): p against p_ref (2 ulp), d(logit), losses and mean
predictions against the fp64 formulas on the device's own p (8 ulp), the classifier's weight / bias gradient against
(N + 2) 2^-24 sum |d(logit) act|, the chain gradients of the live regimes against 1e-4 of each tensor's scale, the latent
objective's floor-regime dz against 1e-4 of max|dz_ref|, the verifier's encoder gradients against the restatement's bound.
The checks that are exact (p == 0 / 0.5 / 1, zero arenas, losses of 100 / 90 / 0, accuracies, bit-for-bit contracts) have no
margin and are not listed: the tests assert them.  Needs the GPU.

    python profiles/saturated_heads_margins.py [--out profiles/saturated_heads_margins.json]"""
import argparse
import itertools
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "saturated_heads_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("saturated_heads_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import test_saturated_heads_gpu as T

    for dtype, variant, batch in itertools.product(("f32", "bf16", "f16"), ("trainer", "ablation"), (T.BATCH_PARTIALS, T.BATCH_STORED)):
        T.test_head_sweep_in_the_step(dtype, variant, batch)
    for kind, b in itertools.product(("f32", "bf16", "f16", "sn"), (-95.0, 25.0)):
        T.test_dead_regimes_through_the_chain(kind, b)
    for b in (-60.0, -35.0, -27.0, 10.0):
        T.test_live_regimes_through_the_chain(b)
    for sn in (False, True):
        T.test_latent_objective_at_saturated_scores(sn)
    for use_c in (True, False):
        T.test_verifier_head_sweep(use_c)
    worst = max((v for row in T.MARGINS.values() for v in row.values()), default=0.0)
    out = {"unit": "observed worst fraction of the bound the test asserts (<= 1)",
           "bounds": {"p": "2 ulp of headcommon.p_ref", "dlogit / losses / means / realism_term / bce": "8 ulp of the fp64 formulas on the device's p",
                      "cls_weight_grad / cls_bias_grad / cls3_bias_grad": "(N + 2) 2^-24 sum |d(logit) act| (+ 8 ulp per pair for the verifier)",
                      "d_grads / g_grads": "1e-4 of each tensor's scale (hipcommon.grad_scales)",
                      "dz_floor_regime": "1e-4 of max|dz_ref|", "encoder_grads": "min(32 x fp32-vs-fp64 of the restatement, 1e-4)"},
           "sweep": list(T.H.X0), "worst": worst, "cases": T.MARGINS}
    assert worst <= 1.0
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
