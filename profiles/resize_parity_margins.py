"""Writes profiles/resize_parity_margins.json: what tests/test_resize_gpu.py bounds, as measured -- per shape the worst error
of resize_f32 and of resize_f32_adjoint against the fp64 dense maps of Pillow's double weights, and the difference of the two
sides of <R x, y> = <x, R^T y>, each as a ratio to the derived bound the test asserts (4 (ksize + 2) 2^-24 max|x| per
element; the test file's docstring derives it); the differing bytes of resize_u8 against Pillow over the test's shapes and
contents (0, or the test fails); and the largest distance of the fp32 path from the byte path in bytes (bound 1.01).
Needs the GPU.

    python profiles/resize_parity_margins.py [--out profiles/resize_parity_margins.json]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize_parity_margins.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resize_parity_margins.py measures on the MI355X: no ROCm device found")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import resizecommon as RC
    import test_resize_gpu as T
    from signature_gan_amd import resize

    out = {"bound": "4 * (ksize + 2) * 2^-24 * max|input| per element", "fp32": [T.f32_margins(s) for s in T.F32_SHAPES]}
    differing, images = 0, 0
    for shape in T.U8_SHAPES:
        for kind in T.KINDS:
            b = RC.contents(kind, shape, seed=shape[1] * 7 + shape[2])
            differing += int((resize.resize_u8(torch.from_numpy(b).to(T.DEV)).cpu().numpy() != RC.pillow_resize(b)).sum())
            images += shape[0]
    out["resize_u8_vs_pillow"] = {"images": images, "differing_bytes": differing}
    b = torch.from_numpy(RC.contents("strokes", (3, 128, 128), seed=6)).to(T.DEV)
    gap = (resize.resize_f32(b.float() / 127.5 - 1.0) - (resize.resize_u8(b).float() / 127.5 - 1.0)).abs().max()
    out["fp32_path_vs_byte_path"] = {"worst_bytes": float(gap) * 127.5, "bound_bytes": 1.01}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
