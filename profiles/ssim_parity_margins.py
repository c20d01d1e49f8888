#!/usr/bin/env python3
"""How much of the SSIM tests' bound the kernel uses on the MI355X.

    python profiles/ssim_parity_margins.py [--out profiles/ssim_parity_margins.json]

Per size of tests/test_ssim_gpu.py, over the pairs its tests score (tests/ssimcommon.World: A x B and A x A):
  "fp32_restatement_deviation"  largest |plain-fp32 numpy restatement - float64 restatement|
  "bound"                       16 x that: what the tests allow
  "kernel_deviation"            largest |ssim_matrix on the device - float64 restatement|
  "ratio"                       kernel_deviation / bound
  "kernel_over_fp32"            kernel_deviation / fp32_restatement_deviation: 1 means the kernel is as far from the exact value
                                as numpy's fp32 is
Needs the GPU; there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssimcommon as SC  # noqa: E402

import signature_gan_amd  # noqa: E402,F401
from signature_gan_amd import ssim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_parity_margins.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    res = {"device_name": torch.cuda.get_device_name(0), "margin": SC.MARGIN, "sizes": {}}
    for h, w in SC.SIZES:
        world = SC.world(h, w)
        sa, sb = ssim.SsimSet(torch.from_numpy(world.a).cuda()), ssim.SsimSet(torch.from_numpy(world.b).cuda())
        ab, aa = ssim.ssim_matrix(sa, sb).cpu().numpy().astype(np.float64), ssim.ssim_matrix(sa).cpu().numpy().astype(np.float64)
        err = max(float(np.abs(ab - world.ab64).max()), float(np.abs(aa - world.aa64).max()))
        res["sizes"][f"{h}x{w}"] = {"pairs": int(ab.size + aa.size), "fp32_restatement_deviation": world.fp32_deviation,
                                    "bound": world.bound, "kernel_deviation": err, "ratio": err / world.bound,
                                    "kernel_over_fp32": err / world.fp32_deviation}
        print(f"{h}x{w}", json.dumps(res["sizes"][f"{h}x{w}"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
