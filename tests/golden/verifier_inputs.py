"""Deterministic synthetic inputs of the signature-verifier fixtures (DATA GENERATION only, like inputs.py): the Siamese
network's state, the two image batches of a case and the score / label vector the metrics are pinned on.  The fixtures
store only the reference's OUTPUTS for these; both sides regenerate the inputs from (seed, stream)."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

import inputs as I

SEED = dict(state=707, state2=708, x1=31, x2=32, metrics=55)
CASES = [(1, 128),      # the smallest batch
         (3, 128),      # 6 images: a ragged M tile in fc1
         (33, 128),     # 66 images: more than one 64-row fc1 tile plus a tail, 528 conv2 tiles
         (3, 40)]       # an embedding width that is not a multiple of 32
STAGES = (("pool1", (32, 32, 32)), ("pool2", (64, 16, 16)), ("pool3", (128, 8, 8)), ("fc1", (512,)))


def case_name(n_pairs: int, e: int) -> str:
    return f"golden_verifier_p{n_pairs}_e{e}"


def state_specs(e: int = 128) -> "OrderedDict[str, tuple]":
    """SiameseNetwork(e).state_dict() order: name -> (shape, kind)."""
    s = OrderedDict()
    for i, (co, ci, k) in enumerate(((32, 1, 5), (64, 32, 5), (128, 64, 3)), start=1):
        s[f"encoder.conv{i}.weight"] = ((co, ci, k, k), "param")
        s[f"encoder.conv{i}.bias"] = ((co,), "param")
        s[f"encoder.bn{i}.weight"] = ((co,), "bn_gamma")
        s[f"encoder.bn{i}.bias"] = ((co,), "bn_beta")
        s[f"encoder.bn{i}.running_mean"] = ((co,), "bn_mean")
        s[f"encoder.bn{i}.running_var"] = ((co,), "bn_var")
        s[f"encoder.bn{i}.num_batches_tracked"] = ((), "counter")
    s["encoder.fc1.weight"] = ((512, 8192), "param")
    s["encoder.fc1.bias"] = ((512,), "param")
    s["encoder.fc2.weight"] = ((e, 512), "param")
    s["encoder.fc2.bias"] = ((e,), "param")
    s["classifier.0.weight"] = ((64, e), "head")
    s["classifier.0.bias"] = ((64,), "head")
    s["classifier.3.weight"] = ((1, 64), "head")
    s["classifier.3.bias"] = ((1,), "head")
    return s


def gen_state(e: int = 128, seed: int = SEED["state"]) -> "OrderedDict[str, np.ndarray]":
    out = OrderedDict()
    for name, (shape, kind) in state_specs(e).items():
        g = I.rng(seed, name)
        if kind == "counter":
            out[name] = np.array(7, dtype=np.int64)
        elif kind == "bn_gamma":
            out[name] = (1.0 + 0.1 * g.standard_normal(shape)).astype(np.float32)
        elif kind in ("bn_beta", "bn_mean"):
            out[name] = (0.1 * g.standard_normal(shape)).astype(np.float32)
        elif kind == "bn_var":
            out[name] = g.uniform(0.5, 1.5, shape).astype(np.float32)
        elif kind == "head":                              # wide enough that the scores spread
            out[name] = (0.5 * g.standard_normal(shape)).astype(np.float32)
        else:
            out[name] = (0.05 * g.standard_normal(shape)).astype(np.float32)
    return out


def normalize_bytes(b: np.ndarray) -> np.ndarray:
    """ToTensor then Normalize([0.5], [0.5]) in fp32: the exact fp32 twin of a uint8 image."""
    v = b.astype(np.float32) / np.float32(255.0)
    return (v - np.float32(0.5)) / np.float32(0.5)


def gen_x1(n: int, seed: int = SEED["x1"]) -> np.ndarray:
    """Uniform in [-1, 1]: every padding border carries signal."""
    return I.rng(seed, "x1").uniform(-1.0, 1.0, (n, 1, 64, 64)).astype(np.float32)


def gen_x2_bytes(n: int, seed: int = SEED["x2"]) -> np.ndarray:
    """Stroke-like uint8 (n, 64, 64): white background, about 10 % ink of random darkness."""
    g = I.rng(seed, "x2")
    ink = g.uniform(0.0, 1.0, (n, 64, 64)) < 0.10
    dark = g.integers(0, 160, (n, 64, 64), dtype=np.int64)
    return np.where(ink, dark, 255).astype(np.uint8)


def gen_x2(n: int, seed: int = SEED["x2"]) -> np.ndarray:
    return normalize_bytes(gen_x2_bytes(n, seed))[:, None]


def gen_scores(seed: int = SEED["metrics"]):
    """(y_true, y_scores, threshold) of 200 pairs: scores rounded to two decimals (ties, also across the classes), a run of 12
    genuine pairs with distinct top scores and a run of 9 forgeries with distinct bottom scores (consecutive thresholds that
    move only TPR / only FPR: the collinear points roc_curve drops)."""
    g = I.rng(seed, "scores")
    y = (g.uniform(0.0, 1.0, 179) < 0.5).astype(np.float64)
    s = np.round(np.clip(0.5 + 0.18 * (2 * y - 1) + 0.2 * g.standard_normal(179), 0.02, 0.9), 2)
    y = np.concatenate([y, np.ones(12), np.zeros(9)])
    s = np.concatenate([s, 0.95 + 0.004 * np.arange(12), 0.001 + 0.002 * np.arange(9)])
    p = g.permutation(y.size)
    return y[p], s[p], 0.5
