"""Nearest-neighbour metrics between two sets of feature vectors that stay on the device.

One number (utils/frechet.py) cannot tell a Generator that has collapsed onto a few good signatures from one that covers
the data badly, and it says nothing about a generated signature that is a near copy of a training one.  The figures that
do are k-nearest-neighbour queries between the two sets of embeddings:

* improved precision / recall (Kynkaanniemi et al. 2019): the fraction of generated samples inside the real set's
  manifold -- the union of the balls around every real sample that reach to its k-th nearest real neighbour -- and the
  fraction of real samples inside the generated set's;
* density / coverage (Naeem et al. 2020): in how many real balls a generated sample lies on average, over k, and the
  fraction of real samples whose ball holds at least one generated sample;
* nearest-real distances: from every generated sample to its nearest real one, against the real set's own leave-one-out
  nearest-neighbour distances.  A median ratio well below 1 is the memorisation warning.

``knn`` and ``ball_count`` (include/siggan_neighbors.h, csrc/neighbors.hip) answer the queries in fp64 on the device
without forming the distance matrix; ``manifold_metrics`` makes six launches and brings only k-lists and counts to the
host, where ``manifold_from_neighbors`` -- pure numpy, the definitions in one place -- reduces them."""
from typing import Any, Dict, Tuple

import numpy as np
import torch

from .. import _call, _lib
from .._call import ptr, stream

CLOSEST = 5                                                 # how many generated -> real pairs ``nearest_real`` lists


def _check_sets(q: torch.Tensor, r: torch.Tensor) -> torch.device:
    for name, t in (("q", q), ("r", r)):
        _call.check_rows(name, t, torch.float32, "(n, dim)")
    if r.device != q.device or r.shape[1] != q.shape[1]:
        raise ValueError(f"q {tuple(q.shape)} on {q.device} and r {tuple(r.shape)} on {r.device} must share device and dim")
    return q.device


def knn(q: torch.Tensor, r: torch.Tensor, k: int, exclude_self: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(dist2 fp64 (nq, k), index int32 (nq, k)): for every row of q (nq, dim) the k smallest squared Euclidean distances
    to the rows of r (nr, dim), ascending, equal distances by ascending row number.  ``exclude_self``: q and r are the same
    set and row i is not its own neighbour.  Both fp32 contiguous on one ROCm device; nothing synchronises the host."""
    dev = _check_sets(q, r)
    k = int(k)
    if not 1 <= k <= _lib.KNN_MAX_K:
        raise ValueError(f"k = {k} outside [1, {_lib.KNN_MAX_K}]")
    dist2 = torch.empty(q.shape[0], k, dtype=torch.float64, device=dev)
    index = torch.empty(q.shape[0], k, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().siggan_knn(dev.index, ptr(q), q.shape[0], ptr(r), r.shape[0], q.shape[1], k, 1 if exclude_self else 0,
                                      ptr(dist2), ptr(index), stream(dev)))
    return dist2, index


def ball_count(q: torch.Tensor, r: torch.Tensor, radius2: torch.Tensor) -> torch.Tensor:
    """int32 (nq): in how many of the balls around the rows of r -- squared radii ``radius2``, fp64 (nr) -- each row of q
    lies (d2 <= radius2, the distances ``knn`` gives)."""
    dev = _check_sets(q, r)
    _call.check_vector("radius2", radius2, torch.float64, r.shape[0], dev)
    count = torch.empty(q.shape[0], dtype=torch.int32, device=dev)
    _lib.check(_lib.load().siggan_ball_count(dev.index, ptr(q), q.shape[0], ptr(r), r.shape[0], q.shape[1], ptr(radius2), ptr(count),
                                             stream(dev)))
    return count


def _check_sizes(n_real: int, n_fake: int, k: int) -> None:
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if n_real <= k or n_fake <= k:
        raise ValueError(f"the k-th neighbour inside a set needs more than k = {k} samples per set, got {n_real} real and "
                         f"{n_fake} generated")


def manifold_from_neighbors(k: int, radius2_real, radius2_fake, fake_in_real, real_in_fake, real_to_fake_d2, fake_to_real_d2,
                            fake_to_real_index, real_loo_d2) -> Dict[str, Any]:
    """The metric definitions on ready neighbour data (numpy, no device).  With n_real real and n_fake generated samples:

    radius2_real (n_real), radius2_fake (n_fake): squared distance of every sample to its k-th nearest neighbour in its own
    set, itself left out; fake_in_real (n_fake): in how many real balls each generated sample lies; real_in_fake (n_real):
    the converse; real_to_fake_d2 (n_real) / fake_to_real_d2, fake_to_real_index (n_fake): squared distance to (and row
    number of) the nearest sample of the other set; real_loo_d2 (n_real): squared distance of every real sample to its
    nearest other real sample."""
    k = int(k)
    radius2_real, radius2_fake = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (radius2_real, radius2_fake))
    n_real, n_fake = radius2_real.size, radius2_fake.size
    _check_sizes(n_real, n_fake, k)
    fake_in_real, real_in_fake = np.asarray(fake_in_real).reshape(-1), np.asarray(real_in_fake).reshape(-1)
    real_to_fake_d2, fake_to_real_d2, real_loo_d2 = (np.asarray(a, dtype=np.float64).reshape(-1)
                                                     for a in (real_to_fake_d2, fake_to_real_d2, real_loo_d2))
    fake_to_real_index = np.asarray(fake_to_real_index).reshape(-1)
    for name, a, n in (("fake_in_real", fake_in_real, n_fake), ("real_in_fake", real_in_fake, n_real),
                       ("real_to_fake_d2", real_to_fake_d2, n_real), ("fake_to_real_d2", fake_to_real_d2, n_fake),
                       ("fake_to_real_index", fake_to_real_index, n_fake), ("real_loo_d2", real_loo_d2, n_real)):
        if a.size != n:
            raise ValueError(f"{name} has {a.size} entries, expected {n}")
    to_real, loo = np.sqrt(fake_to_real_d2), np.sqrt(real_loo_d2)
    median, loo_median = float(np.median(to_real)), float(np.median(loo))
    order = np.lexsort((np.arange(n_fake), to_real))[:CLOSEST]           # by distance, equal ones by generated index
    return {
        "k": k, "n_real": n_real, "n_generated": n_fake,
        "radius2_real": radius2_real, "radius2_fake": radius2_fake,
        "precision": float(np.mean(fake_in_real > 0)),
        "recall": float(np.mean(real_in_fake > 0)),
        "density": float(fake_in_real.sum(dtype=np.int64)) / float(k * n_fake),
        "coverage": float(np.mean(real_to_fake_d2 <= radius2_real)),
        "nearest_real": {
            "mean": float(np.mean(to_real)), "median": median, "min": float(np.min(to_real)),
            "real_loo_median": loo_median,
            "ratio_median": median / loo_median if loo_median > 0 else None,
            "closest": [(int(i), int(fake_to_real_index[i]), float(to_real[i])) for i in order],
        },
    }


def manifold_metrics(real_emb: torch.Tensor, fake_emb: torch.Tensor, k: int = 3) -> Dict[str, Any]:
    """Precision, recall, density, coverage and nearest-real distances of two (n, dim) fp32 embedding sets on one ROCm
    device; n_real > k and n_fake > k, else ValueError.  Six launches; k-lists and counts reach the host, the embeddings
    and the distances between them do not.  Keys: ``manifold_from_neighbors``."""
    k = int(k)
    n_real = real_emb.shape[0] if isinstance(real_emb, torch.Tensor) and real_emb.dim() == 2 else 0
    n_fake = fake_emb.shape[0] if isinstance(fake_emb, torch.Tensor) and fake_emb.dim() == 2 else 0
    _check_sizes(n_real, n_fake, k)
    _check_sets(fake_emb, real_emb)
    real_d2, _ = knn(real_emb, real_emb, k, exclude_self=True)           # column 0 is the leave-one-out nearest neighbour
    fake_d2, _ = knn(fake_emb, fake_emb, k, exclude_self=True)
    radius2_real, radius2_fake = real_d2[:, k - 1].contiguous(), fake_d2[:, k - 1].contiguous()
    fake_in_real = ball_count(fake_emb, real_emb, radius2_real)
    real_in_fake = ball_count(real_emb, fake_emb, radius2_fake)
    real_to_fake_d2, _ = knn(real_emb, fake_emb, 1)
    fake_to_real_d2, fake_to_real_index = knn(fake_emb, real_emb, 1)
    host = [t.cpu().numpy() for t in (radius2_real, radius2_fake, fake_in_real, real_in_fake, real_to_fake_d2, fake_to_real_d2,
                                      fake_to_real_index, real_d2[:, 0])]
    return manifold_from_neighbors(k, *host)
