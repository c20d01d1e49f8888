"""Diversity-aware selection from a pool of feature vectors that stays on the device.

Ranking a generated pool by the Discriminator's score (Engine.select_topk) concentrates on whatever mode the Discriminator
likes best, and near-duplicates pass together because their scores are nearly equal.  The metrics of utils/neighbors.py
measure that; this module acts on it: ``select_diverse`` (include/siggan_diverse.h, csrc/diverse.hip) picks, greedily, the
rows that are mutually farthest apart -- every pick is the eligible row farthest, in fp64, from everything picked so far
and from an optional set of anchors -- and may stop early once nothing new is far enough from what is kept.  What may be
picked at all is a mask: ``eligibility`` builds it from the realism scores (the better part of the pool, by select_topk's own
order) and from the distance to the nearest real sample (no near copies).  ``diversity_summary`` -- pure numpy, the
definitions in one place -- turns what a run fetched into its report.

Whether a verifier trained on a set selected this way is more accurate than one trained on the top of the ranking is not
measured here."""
import math
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch

from .. import _lib
from .._call import check_rows, check_vector, ptr, stream
from .neighbors import _check_sets


def select_diverse(x: torch.Tensor, n_select: int, eligible: Optional[torch.Tensor] = None,
                   anchor_d2: Optional[torch.Tensor] = None, first: Optional[int] = None, min_separation: float = 0.0
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(order int32 (n_select,), gain2 fp64 (n_select,), count int32 (1,), min_d2 fp64 (n,)), all on x's device: greedy
    farthest-point selection among the rows of x (n, dim) fp32 (siggan_select_diverse; the header states the semantics).
    Pick t is the row with ``eligible`` (uint8 (n,), None: all) set and not yet picked whose squared distance to the nearest
    earlier pick -- and to the nearest anchor, ``anchor_d2`` fp64 (n,) -- is largest, equal values by the lower row;
    ``first``: the row taken as pick 0 whatever the mask says.  gain2[t] is that squared distance (+inf for the first pick
    without anchors).  The run stops when no row is left or the best squared distance falls below ``min_separation`` ** 2:
    count is the number of picks, order is -1 and gain2 0.0 beyond it.  min_d2: every row's squared distance to the nearest
    pick or anchor.  The workspace is this call's own; nothing synchronises the host."""
    dev = _check_sets(x, x)
    n, dim = x.shape
    n_select = int(n_select)
    if eligible is not None:
        check_vector("eligible", eligible, torch.uint8, n, dev)
    if anchor_d2 is not None:
        check_vector("anchor_d2", anchor_d2, torch.float64, n, dev)
    min_separation = float(min_separation)
    if not min_separation >= 0.0:
        raise ValueError(f"min_separation must be >= 0, got {min_separation}")
    lib = _lib.load()
    size = int(lib.siggan_select_diverse_workspace(n))
    workspace = torch.empty(max(size, 8) // 8 + 1, dtype=torch.float64, device=dev)
    k = max(n_select, 1)
    order = torch.empty(k, dtype=torch.int32, device=dev)
    gain2 = torch.empty(k, dtype=torch.float64, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    min_d2 = torch.empty(n, dtype=torch.float64, device=dev)
    _lib.check(lib.siggan_select_diverse(dev.index, ptr(x), n, dim, ptr(eligible), ptr(anchor_d2), -1 if first is None else int(first),
                                         n_select, min_separation * min_separation, ptr(order), ptr(gain2), ptr(count), ptr(min_d2),
                                         ptr(workspace), size, stream(dev)))
    return order, gain2, count, min_d2


def eligibility(scores: torch.Tensor, keep_ratio: float, nearest_real_d2: Optional[torch.Tensor] = None, floor2=None) -> torch.Tensor:
    """uint8 (n,) device mask of the rows a diverse selection may pick: the ceil(keep_ratio * n) best of the float32 device
    ``scores`` by Engine.select_topk's own order (equal scores by ascending index, as the realism filter resolves them), and
    -- when both are given -- only rows with ``nearest_real_d2`` (fp64 (n,) device: squared distance to the nearest real
    sample) >= ``floor2`` (a number or a 0-d device tensor).  Nothing synchronises the host."""
    from ..engine import Engine
    check_rows("scores", scores, torch.float32, "(n >= 1,)", shape=(None,), min_rows=1)
    n = scores.numel()
    keep_ratio = float(keep_ratio)
    if not 0.0 < keep_ratio <= 1.0:
        raise ValueError(f"keep_ratio must be in (0, 1], got {keep_ratio}")
    if (nearest_real_d2 is None) != (floor2 is None):
        raise ValueError("nearest_real_d2 and floor2 come together")
    keep = min(n, max(1, math.ceil(keep_ratio * n)))
    index = Engine.select_topk(scores, keep)
    mask = torch.zeros(n, dtype=torch.uint8, device=scores.device)
    mask[index.long()] = 1
    if nearest_real_d2 is not None:
        check_vector("nearest_real_d2", nearest_real_d2, torch.float64, n, scores.device)
        mask = mask * (nearest_real_d2 >= floor2).to(torch.uint8)
    return mask.contiguous()


def _nn_stats(nn_d2, realism) -> Dict[str, Any]:
    """{min_nn_distance, mean_nn_distance, mean_realism} of one selection: ``nn_d2`` its members' squared distances to their
    nearest other member (None or empty: fewer than two members, the two distances are None)."""
    realism = np.asarray(realism, dtype=np.float64).reshape(-1)
    d = None if nn_d2 is None else np.sqrt(np.asarray(nn_d2, dtype=np.float64).reshape(-1))
    has = d is not None and d.size > 0
    return {"min_nn_distance": float(d.min()) if has else None, "mean_nn_distance": float(d.mean()) if has else None,
            "mean_realism": float(realism.mean()) if realism.size else None}


def diversity_summary(pool: int, eligible: int, requested: int, order, gain2, count: int, realism, nearest_real_d2=None,
                      coverage_d2: Optional[float] = None, selection_nn_d2=None, top_realism=(), top_nn_d2=None) -> Dict[str, Any]:
    """The report of a diverse selection from fetched data (numpy, no device).  ``pool`` rows of which ``eligible`` could be
    picked and ``requested`` were asked for; ``order`` / ``gain2`` / ``count`` as select_diverse returns them; ``realism`` and
    ``nearest_real_d2`` (None: no real set) of the ``count`` picks in pick order; ``coverage_d2``: the largest final min_d2
    over the eligible rows (None: there were none); ``selection_nn_d2`` / ``top_nn_d2``: inside this selection and inside the
    plain top-by-realism selection of the same pool, every member's squared distance to its nearest other member (knn with
    exclude_self; None with fewer than two members); ``top_realism``: the scores of that top selection.

    stopped_by: 'count' -- as many as requested --, else 'exhausted' -- every eligible row was picked --, else 'separation'
    -- the best remaining row was closer than min_separation.  gain: sqrt(gain2), None for +inf (a first pick without
    anchors)."""
    count = int(count)
    order = np.asarray(order).reshape(-1)[:count]
    gain2 = np.asarray(gain2, dtype=np.float64).reshape(-1)[:count]
    realism = np.asarray(realism, dtype=np.float64).reshape(-1)
    if order.size != count or gain2.size != count or realism.size != count:
        raise ValueError(f"order, gain2 and realism must hold the {count} picks")
    if count and int(order.min()) < 0:
        raise ValueError("order holds -1 inside the first count picks")
    near = None if nearest_real_d2 is None else np.sqrt(np.asarray(nearest_real_d2, dtype=np.float64).reshape(-1))
    if near is not None and near.size != count:
        raise ValueError(f"nearest_real_d2 must hold the {count} picks")
    stopped_by = "count" if count >= int(requested) else ("exhausted" if count >= int(eligible) else "separation")
    picks = [{"pool_index": int(order[t]), "realism": float(realism[t]),
              "gain": float(np.sqrt(gain2[t])) if np.isfinite(gain2[t]) else None,
              "nearest_real": None if near is None else float(near[t])} for t in range(count)]
    return {"pool": int(pool), "eligible": int(eligible), "requested": int(requested), "selected": count, "stopped_by": stopped_by,
            "picks": picks, "coverage_radius": None if coverage_d2 is None else float(np.sqrt(coverage_d2)),
            "diverse": _nn_stats(selection_nn_d2, realism), "top_n": _nn_stats(top_nn_d2, top_realism)}
