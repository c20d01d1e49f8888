"""Hard-pair mining for the Siamese verifier's trainer, on the device.

The reference draws its training pairs once, at random (``SignaturePairDataset._generate_pairs``), and reuses that list every
epoch; after a few epochs almost all of them are easy.  The pairs that decide the equal-error rate are the impostors the head
scores HIGHEST and the genuine pairs it scores LOWEST -- among the impostors the GAN's own signatures, which enter the trainer as
the ``_synthetic_`` writer and serve only as negatives.  Everything mining needs is already in HBM: the device input pipeline
keeps every decoded file as bytes (``verifier_data.DevicePairLoader``), ``embed_u8`` embeds them in eval mode, and
``SiameseNetwork.pair_topk`` (include/siggan_verifier_topk.h) takes every signature's k hardest impostors and k hardest genuine
partners out of one pass over all pairs.  Only the (N, k) index arrays cross to the host.

``MiningPairLoader`` is a ``DevicePairLoader`` whose cache holds the whole signature table and whose epochs run over the
dataset's pairs plus the pairs mined last; before the first ``remine`` it is a ``DevicePairLoader`` bit for bit.  Whether mined
pairs improve accuracy is not measured here; the trainer's ``--hard_mining`` is off by default.

The selection (``hard_pairs_from_topk``) and the table (``signature_table``) are pure CPU; the rest needs a ROCm device.
"""
from typing import Iterable, List, Tuple

import numpy as np
import torch
from torch.utils.data import Subset

from .verifier_data import DevicePairLoader, _pairs_of

SYNTHETIC = "_synthetic_"


def _base_dataset(ds):
    while isinstance(ds, Subset):
        ds = ds.dataset
    return ds


def signature_table(pairs_dataset) -> Tuple[List, np.ndarray, np.ndarray]:
    """(files, writer ids int32 (N,), synthetic bool (N,)) of every file of the SignaturePairDataset under ``pairs_dataset`` (the
    dataset itself or nested Subsets of it), in ``user_signatures``' order: writer w of that dict gets id w."""
    files, ids, synthetic = [], [], []
    for w, (user, sigs) in enumerate(_base_dataset(pairs_dataset).user_signatures.items()):
        files += list(sigs)
        ids += [w] * len(sigs)
        synthetic += [user == SYNTHETIC] * len(sigs)
    return files, np.asarray(ids, np.int32), np.asarray(synthetic, bool)


def hard_pairs_from_topk(imp_idx, gen_idx, anchor_ok, exclude: Iterable = ()) -> np.ndarray:
    """The mined pair list, (H, 3) int64 rows (i, j, label): per anchor row i with ``anchor_ok[i]``, (i, j, 0) for every impostor
    index j >= 0 of row i, then (i, j, 1) for every genuine index j >= 0 (-1 pads a short list).  The reference never anchors on
    the synthetic writer, so those rows are candidates only.  An unordered pair is kept once, at its first occurrence in anchor
    order; the unordered pairs of ``exclude`` ((i, j) or (i, j, label) rows -- the validation split's pairs, so that mining does
    not hand the validation set to the optimiser) are dropped."""
    imp_idx, gen_idx = np.asarray(imp_idx), np.asarray(gen_idx)
    anchor_ok = np.asarray(anchor_ok, bool)
    n = len(anchor_ok)
    if imp_idx.shape[0] != n or gen_idx.shape[0] != n or imp_idx.ndim != 2 or gen_idx.ndim != 2:
        raise ValueError(f"the index arrays must be ({n}, k), got {imp_idx.shape} and {gen_idx.shape}")
    seen = {(min(int(e[0]), int(e[1])), max(int(e[0]), int(e[1]))) for e in exclude}
    out = []
    for i in np.flatnonzero(anchor_ok):
        for row, label in ((imp_idx[i], 0), (gen_idx[i], 1)):
            for j in row:
                j = int(j)
                key = (min(int(i), j), max(int(i), j))
                if j < 0 or key in seen:
                    continue
                seen.add(key)
                out.append((int(i), j, label))
    return np.asarray(out, np.int64).reshape(-1, 3)


def mine_hard_pairs(model, cache_u8: torch.Tensor, ids: torch.Tensor, anchor_ok, k_impostor: int, k_genuine: int,
                    exclude: Iterable = ()) -> np.ndarray:
    """``hard_pairs_from_topk`` of the model's current weights over the (N, 64, 64) uint8 device cache: ``embed_u8`` in eval mode
    (the context embeds ``max_images`` images per call; the model's mode is restored), one ``pair_topk(same_set=True)`` with
    ids (N,) int32 on the device for each row's ``k_impostor`` highest-scoring impostors and ``k_genuine`` lowest-scoring genuine
    partners (0 skips a class), and the selection on the host.  Only the index arrays are read back."""
    k_impostor, k_genuine = int(k_impostor), int(k_genuine)
    if k_impostor < 0 or k_genuine < 0 or k_impostor + k_genuine == 0:
        raise ValueError(f"k_impostor and k_genuine must be >= 0 and not both 0, got {k_impostor} and {k_genuine}")
    want = tuple(c for c, k in (("impostor", k_impostor), ("genuine", k_genuine)) if k)
    n = cache_u8.shape[0]
    was_training = model.training
    model.eval()
    try:
        emb = model.embed_u8(cache_u8)
        out = model.pair_topk(emb, ids, emb, ids, max(k_impostor, k_genuine), same_set=True, genuine_lowest=True, want=want)
    finally:
        model.train(was_training)
    # a list of k is the head of the list of any larger k
    idx = {c: (out[f"{c}_index"][:, :k].cpu().numpy() if k else np.zeros((n, 0), np.int32))
           for c, k in (("impostor", k_impostor), ("genuine", k_genuine))}
    return hard_pairs_from_topk(idx["impostor"], idx["genuine"], anchor_ok, exclude)


class MiningPairLoader(DevicePairLoader):
    """A DevicePairLoader whose cache holds every file of the signature table (``signature_table`` order) and whose epochs run
    over the dataset's pairs followed by the pairs ``remine`` found last -- planned, augmented and gathered by the same path.
    ``exclude_dataset``: a pair dataset (the validation split) whose pairs are never mined; ``elastic`` / ``elastic_seed``: as
    for DevicePairLoader."""

    def __init__(self, pairs_dataset, batch_size: int, shuffle: bool, augment: bool, k_impostor: int, k_genuine: int = None,
                 exclude_dataset=None, device=None, drop_last: bool = False, elastic=None, elastic_seed: int = 0):
        self.files, ids, synthetic = signature_table(pairs_dataset)
        self._row = {p: r for r, p in enumerate(self.files)}
        super().__init__(pairs_dataset, batch_size, shuffle, augment, device=device, drop_last=drop_last, elastic=elastic,
                         elastic_seed=elastic_seed)
        self.k_impostor = int(k_impostor)
        self.k_genuine = self.k_impostor if k_genuine is None else int(k_genuine)
        self.ids = torch.from_numpy(ids).to(self.device)
        self.anchor_ok = ~synthetic
        self.exclude = [(self._row[p1], self._row[p2]) for p1, p2, _ in _pairs_of(exclude_dataset)] if exclude_dataset is not None else []
        self.mined = np.zeros((0, 3), np.int64)

    def _cache_slots(self, pairs) -> dict:
        return dict(self._row)

    def _epoch_pairs(self):
        if not len(self.mined):
            return self._slots, self._labels
        return (np.concatenate([self._slots, self.mined[:, :2].astype(np.int32)]),
                np.concatenate([self._labels, self.mined[:, 2].astype(np.float32)]))

    def remine(self, model) -> Tuple[int, int, int]:
        """Replaces the mined pairs by those of the model's current weights; returns (pairs, impostor pairs, genuine pairs)."""
        self.mined = mine_hard_pairs(model, self.cache, self.ids, self.anchor_ok, self.k_impostor, self.k_genuine, self.exclude)
        genuine = int(self.mined[:, 2].sum())
        return len(self.mined), len(self.mined) - genuine, genuine
