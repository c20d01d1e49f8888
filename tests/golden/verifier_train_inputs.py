"""Deterministic inputs of the signature-verifier TRAIN-step fixtures (DATA GENERATION only, like verifier_inputs.py): the
cases, labels and dropout keep masks.  State and images are verifier_inputs'; the fixtures store only the reference's
OUTPUTS for these, both sides regenerate the inputs."""
from __future__ import annotations

import numpy as np

import inputs as I
import verifier_inputs as VI

SEED = dict(fc_keep=901, cls_keep=902)
# (pairs, E, steps, labels): two consecutive steps on the first case (Adam bias corrections, moments, the running-statistics
# chain); a ragged fc1 tile and an E that is no multiple of 32 on the second
CASES = [(2, 128, 2, (1.0, 0.0)),
         (3, 40, 1, (1.0, 0.0, 1.0))]
NO_CONTRASTIVE = (3, 40)                 # this case is also stored with use_contrastive = 0 (keys prefixed "nc_")
BIG = (33, 128)                          # no fixture: the restatement on the CPU is the yardstick
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
P_FC, P_CLS = 0.5, 0.3
FULL_BELOW = 4096                        # tensors up to this many elements are stored in full, larger ones at PROBES positions
PROBES = 128
NEAR_TIE = 1e-5                          # decisions whose fp64 margin (relative to the layer's max-abs) is below this are listed
DECISIONS = ("route1", "route2", "route3", "fc1_mask", "cls_mask")


def case_name(n_pairs: int, e: int) -> str:
    return f"golden_verifier_train_p{n_pairs}_e{e}"


def param_names(e: int = 128):
    """SiameseNetwork(e).named_parameters() order."""
    return [k for k, (_, kind) in VI.state_specs(e).items() if kind not in ("bn_mean", "bn_var", "counter")]


def running_names():
    return [f"encoder.bn{i}.running_{s}" for i in (1, 2, 3) for s in ("mean", "var")]


def labels(n_pairs: int) -> np.ndarray:
    for n, _, _, lab in CASES:
        if n == n_pairs:
            return np.asarray(lab, np.float32)
    return (np.arange(n_pairs) % 3 != 1).astype(np.float32)


def fc_keep(n_pairs: int, step: int = 0) -> np.ndarray:
    """(2 * n_pairs, 512) 1 / 0, x1's rows first."""
    return (I.rng(SEED["fc_keep"] + step, "fc_keep").uniform(0.0, 1.0, (2 * n_pairs, 512)) < 1.0 - P_FC).astype(np.float32)


def cls_keep(n_pairs: int, step: int = 0) -> np.ndarray:
    return (I.rng(SEED["cls_keep"] + step, "cls_keep").uniform(0.0, 1.0, (n_pairs, 64)) < 1.0 - P_CLS).astype(np.float32)


def stored_idx(numel: int, name: str):
    """None: the tensor is stored in full; else the flat positions that are."""
    return None if numel <= FULL_BELOW else I.probe_idx(numel, "verifier_train:" + name, PROBES)


def pick(a: np.ndarray, name: str) -> np.ndarray:
    a = np.asarray(a).reshape(-1)
    idx = stored_idx(a.size, name)
    return a.copy() if idx is None else a[idx]
