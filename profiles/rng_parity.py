"""Observed parity of the device's Box-Muller normals on the MI355X: every comparison of tests/test_rng_gpu.py's latent,
op_randn and edge cases -- d32 (numpy float32 against float64 on the same draws), the device's deviation from float64, and
the bound min(32 x d32, 1e-4).

    python profiles/rng_parity.py --out profiles/rng_parity.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)

import torch                                                          # noqa: E402

import rngcommon as R                                                 # noqa: E402
import test_rng_gpu as T                                              # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rng_parity.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    T.PARITY = []
    failed = []

    def run(fn, *args):
        try:
            fn(*args)
        except AssertionError as e:                                   # keep measuring: the record says what missed
            failed.append(f"{fn.__name__}{args}: {e}")

    for b in R.LATENT_BATCHES:
        run(T.test_latents_from_the_fused_fc_kernel, b)
    run(T.test_latents_from_the_generic_fc_kernel_are_the_same_bits)
    run(T.test_staged_step_tables_and_latents)
    for n in R.RANDN_N:
        run(T.test_op_randn, n)
    run(T.test_radius_word_at_u_one_gives_zeros)
    run(T.test_radius_word_at_u_min_gives_the_largest_radius)
    run(T.test_radius_word_at_the_largest_u_below_one)
    ratio = max(c["device_deviation"] / c["d32"] for c in T.PARITY if c["d32"] > 0)
    out = {"device": torch.cuda.get_device_name(0), "rule": "absolute deviation from float64 Box-Muller <= min(32 x d32, 1e-4)",
           "comparisons": len(T.PARITY), "largest_device_deviation": max(c["device_deviation"] for c in T.PARITY),
           "largest_deviation_over_d32": ratio, "failed": failed, "cases": T.PARITY}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("device", "comparisons", "largest_device_deviation", "largest_deviation_over_d32", "failed")},
                     indent=1))


if __name__ == "__main__":
    main()
