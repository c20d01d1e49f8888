"""Shared by tests/test_verifier_data_cpu.py and tests/test_verifier_data_gpu.py: the reference's RandomAffine + flip on one
64x64 image by Pillow itself (the yardstick), a numpy emulation of the kernel contract in include/siggan_verifier_data.h, and
a small synthetic user tree."""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import augment_oracle as A  # noqa: E402

S = 64


def pil_affine(img, angle, tx, ty, scale, flip, fill=0):
    """torchvision's F.affine on a PIL image (one Image.transform(AFFINE, NEAREST)), then the horizontal flip."""
    m = A.tv_inverse_affine_matrix([S * 0.5, S * 0.5], float(angle), [int(tx), int(ty)], float(scale), [0.0, 0.0])
    out = np.asarray(Image.fromarray(img, "L").transform((S, S), Image.AFFINE, m, Image.NEAREST, fillcolor=fill))
    return np.ascontiguousarray(out[:, ::-1]) if flip else out


def emulate(img, prm, tab, fill=0):
    """siggan_pairs_augment's contract for one image: prm (8,) int32, tab (2, 64) int16 or None."""
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    if prm[7] & 1:
        xs = S - 1 - xs                                   # the flip replaces the output column before the lookup
    if prm[0] == 0:
        xin, yin = xs, ys
    elif prm[0] == 1:
        a = prm.astype(np.int64)
        xin, yin = (a[3] + ys * a[2] + xs * a[1]) >> 16, (a[6] + ys * a[5] + xs * a[4]) >> 16
    else:
        if tab is None:
            return np.full((S, S), fill, np.uint8)
        xin, yin = tab[0][xs].astype(np.int64), tab[1][ys].astype(np.int64)
    ok = (xin >= 0) & (xin < S) & (yin >= 0) & (yin < S)
    out = np.full((S, S), fill, np.uint8)
    out[ok] = img[np.where(ok, yin, 0), np.where(ok, xin, 0)][ok]
    return out


def write_users(root, users=3, sigs=3, seed=5):
    """users x sigs sparse-ink 48x96 PNGs under root/user<u>/."""
    rng = np.random.default_rng(seed)
    for u in range(users):
        (root / f"user{u}").mkdir(parents=True)
        for k in range(sigs):
            a = np.where(rng.uniform(size=(48, 96)) < 0.1, rng.integers(0, 128, (48, 96)), 255).astype(np.uint8)
            Image.fromarray(a).save(str(root / f"user{u}" / f"sig{k}.png"))
