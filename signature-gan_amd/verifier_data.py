"""Input pipeline of the Siamese verifier's trainer on the device.

The reference feeds ``train_epoch`` from ``DataLoader(SignaturePairDataset(transform), batch_size, shuffle, num_workers=0)``:
two Pillow decodes, resizes and random transforms per pair, every epoch, in the main process
(signature_verifier_train.py:541-548: Resize -> Grayscale -> RandomAffine(degrees=5, translate=(0.1, 0.1), scale=(0.9, 1.1))
-> RandomHorizontalFlip(p=0.1) -> ToTensor -> Normalize).  Here every distinct file is decoded and resized ONCE into an
(N, 64, 64) uint8 cache resident in HBM; a batch is then one kernel launch (``siggan_pairs_augment``,
include/siggan_verifier_data.h) that gathers and augments both halves of the batch as bytes, and the train step normalises
them on load (SIGGAN_VFMT_U8) with the reference's two fp32 operations.

What is kept from the reference, bit for bit:
  * the order of pairs and every random number: ``iter(loader)`` consumes torch's global generator exactly like
    ``iter(DataLoader(..., shuffle, num_workers=0))`` with that transform does -- the loader's base seed, the RandomSampler's
    seed, then per pair the five draws of image 1 and the five of image 2.  Pinned against the real torch DataLoader in
    tests/test_verifier_data_cpu.py.
  * the pixels: torchvision applies RandomAffine as one Pillow ``Image.transform(AFFINE, NEAREST)`` with fill 0; the host
    tabulates Pillow's own arithmetic (running double sums for an axis-aligned matrix, 16.16 fixed point otherwise) and the
    kernel applies it.  Pinned against Pillow in the same file, the kernel itself in tests/test_verifier_data_gpu.py.
torchvision is not installed in the build image: its glue (the order of the draws in ``RandomAffine.get_params``, the matrix
of ``_get_inverse_affine_matrix``) is written from its published source and is the one UNPINNED piece, as for the GAN's
loader (data_loader_signatures.py).

There is no CPU fallback: the loader needs a ROCm device and the HIP library.  The planning functions are pure CPU.
"""
import math
import dataclasses
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import Subset

from .data_loader_signatures import _scale_tables, _uniform_many
from .warp import WarpSpec, warp_u8

SIZE = 64                                   # the verifier's only image size
FILL = 0                                    # RandomAffine's default fill: corners turn black, as in the reference
DEGREES, TRANSLATE, SCALE, FLIP_P = 5.0, (0.1, 0.1), (0.9, 1.1), 0.1


# ------------------------------------------------------------------------------------------------------------------
# host logic (pure CPU): the epoch plan and the per-image resampling parameters
# ------------------------------------------------------------------------------------------------------------------
def plan_pair_epoch(n: int, batch_size: int, shuffle: bool, drop_last: bool = False, augment: bool = True):
    """Pair order and per-image draws of one pass over n pairs -- what
    ``for b in DataLoader(ds, batch_size, shuffle, num_workers=0, drop_last)`` produces with the reference's train transform,
    consuming torch's global generator the same way (module docstring).  Per image, torchvision's RandomAffine.get_params
    order: angle = uniform_(-5, 5), tx = int(round(uniform_(-6.4, 6.4))), ty likewise, scale = uniform_(0.9, 1.1), no shear
    draw; then RandomHorizontalFlip's torch.rand(1) < 0.1.  ``round`` is Python's (halves to even).

    Returns (batches, draws): batches is a list of lists of pair indices; draws is None without ``augment`` (then only the
    base seed, and the sampler's seed if ``shuffle``, are consumed), else a dict of (pairs, 2) arrays in batch order, column 0
    for image 1: angle / scale float64, tx / ty int64, flip bool."""
    torch.empty((), dtype=torch.int64).random_()                    # the loader's base seed (unused with num_workers=0)
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
        perm = torch.randperm(n, generator=g).tolist()
    else:
        perm = list(range(n))
    nb = n // batch_size if drop_last else (n + batch_size - 1) // batch_size
    batches = [perm[b * batch_size:(b + 1) * batch_size] for b in range(nb)]
    total = sum(len(b) for b in batches)
    if not augment:
        return batches, None
    max_dx, max_dy = float(TRANSLATE[0] * SIZE), float(TRANSLATE[1] * SIZE)
    lo = [-DEGREES, -max_dx, -max_dy, SCALE[0], 0.0]
    hi = [DEGREES, max_dx, max_dy, SCALE[1], 1.0]
    d = _uniform_many(None, lo, hi, 2 * total).reshape(total, 2, 5) if total else np.zeros((0, 2, 5))
    return batches, {"angle": d[:, :, 0], "tx": np.rint(d[:, :, 1]).astype(np.int64), "ty": np.rint(d[:, :, 2]).astype(np.int64),
                     "scale": d[:, :, 3], "flip": d[:, :, 4].astype(np.float32) < np.float32(FLIP_P)}


def inverse_affine_matrix(angle: float, tx: float, ty: float, scale: float) -> List[float]:
    """torchvision's functional._get_inverse_affine_matrix([32.0, 32.0], angle, [tx, ty], scale, shear=[0, 0]): the six numbers
    F.affine hands to Pillow's Image.transform(AFFINE) -- output (x, y) reads input (m0 x + m1 y + m2, m3 x + m4 y + m5)."""
    rot = math.radians(angle)
    sx = sy = math.radians(0.0)
    cx = cy = SIZE * 0.5
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / scale for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def build_pair_params(angle, tx, ty, scale, flip) -> Tuple[np.ndarray, np.ndarray]:
    """Per-image kernel parameters for flat arrays of draws: prm (n, 8) int32 and tab (n, 2, 64) int16 (layout in
    include/siggan_verifier_data.h).  Pillow's own path choice: an axis-aligned matrix (m[1] == 0 and m[3] == 0) goes through
    ImagingScaleAffine's per-axis positions (mode 2), anything else through affine_fixed's 16.16 arithmetic (mode 1)."""
    angle, scale = np.asarray(angle, np.float64).reshape(-1), np.asarray(scale, np.float64).reshape(-1)
    tx, ty, flip = np.asarray(tx).reshape(-1), np.asarray(ty).reshape(-1), np.asarray(flip, bool).reshape(-1)
    n = len(angle)
    prm = np.zeros((n, 8), np.int32)
    tab = np.full((n, 2, SIZE), -1, np.int16)
    m = np.array([inverse_affine_matrix(float(angle[i]), float(tx[i]), float(ty[i]), float(scale[i])) for i in range(n)],
                 np.float64).reshape(n, 6)
    axis = (m[:, 1] == 0) & (m[:, 3] == 0)
    prm[:, 0] = np.where(axis, 2, 1)
    if axis.any():
        r = m[axis]
        tab[axis, 0], tab[axis, 1] = _scale_tables(r[:, 0], r[:, 2], r[:, 4], r[:, 5], SIZE)
    if not axis.all():                                      # affine_fixed: FIX(v) = floor(v * 65536 + 0.5)
        r = m[~axis]
        fix = lambda v: np.floor(v * 65536.0 + 0.5).astype(np.int64)
        cols = [fix(r[:, 0]), fix(r[:, 1]), fix(r[:, 2] + r[:, 0] * 0.5 + r[:, 1] * 0.5),
                fix(r[:, 3]), fix(r[:, 4]), fix(r[:, 5] + r[:, 3] * 0.5 + r[:, 4] * 0.5)]
        prm[~axis, 1:7] = np.stack(cols, 1).astype(np.int32)
    prm[flip, 7] |= 1
    return prm, tab


# ------------------------------------------------------------------------------------------------------------------
# the device loader
# ------------------------------------------------------------------------------------------------------------------
def _pairs_of(ds):
    """(path1, path2, label) of every item of a SignaturePairDataset or of (nested) Subsets of one, in item order."""
    if isinstance(ds, Subset):
        inner = _pairs_of(ds.dataset)
        return [inner[i] for i in ds.indices]
    return list(ds.pairs)


class DevicePairLoader:
    """Iterable over (x1, x2, labels) batches in HBM -- x1 / x2 uint8 (B, 64, 64) views of one (2B, 64, 64) tensor, labels fp32
    (B,) -- for ``train_epoch`` / ``evaluate``; ``len``, ``.dataset`` and ``.batch_size`` as torch's DataLoader.
    ``pairs_dataset`` is a SignaturePairDataset or a torch.utils.data.Subset of one (what random_split returns).

    ``elastic``: a ``warp.WarpSpec`` (None: off, and the loader is what it was without it).  With ``augment``, every batch's
    2m augmented rows then go through one more launch, the smooth random warp of ``warp.warp_u8`` with the loader's FILL,
    into a second buffer.  A row's draw id is epoch * 2^32 + its running number in the epoch (rows in batch order, a
    batch's m first images before its m second ones); the epoch is a count of ``iter()`` calls the loader keeps, from 0;
    ``elastic_seed`` is the warp's seed.  torch's generator is not consumed."""

    def __init__(self, pairs_dataset, batch_size: int, shuffle: bool, augment: bool,
                 device: Union[str, torch.device, None] = None, drop_last: bool = False, elastic: Optional[WarpSpec] = None,
                 elastic_seed: int = 0):
        from . import _lib
        from .signature_verifier_eval import load_uint8
        self.lib = _lib.load()                               # raises if the HIP library is missing
        self._check = _lib.check
        dev = torch.device(device if device is not None else "cuda")
        if dev.type != "cuda":
            raise RuntimeError("the input pipeline runs on a ROCm device (no CPU fallback); got device=%r" % (device,))
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if batch_size < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if elastic is not None:
            if not isinstance(elastic, WarpSpec):
                raise ValueError(f"elastic must be a WarpSpec, got {type(elastic).__name__}")
            elastic = dataclasses.replace(elastic.check(), fill=FILL)
        self.elastic, self.elastic_seed, self.epoch = elastic, int(elastic_seed), 0
        self.device, self.dataset = dev, pairs_dataset
        self.batch_size, self.shuffle, self.augment, self.drop_last = int(batch_size), bool(shuffle), bool(augment), bool(drop_last)
        pairs = _pairs_of(pairs_dataset)
        slot = self._cache_slots(pairs)
        cache = np.zeros((max(len(slot), 1), SIZE, SIZE), np.uint8)
        for p, k in slot.items():                            # decode + resize once; an unreadable file raises, as in the reference
            cache[k] = load_uint8(p)
        self.cache = torch.from_numpy(cache).to(dev)
        self._slots = np.array([[slot[p1], slot[p2]] for p1, p2, _ in pairs], np.int32).reshape(len(pairs), 2)
        self._labels = np.array([float(y) for _, _, y in pairs], np.float32)

    def _cache_slots(self, pairs) -> dict:
        """file -> row of the cache: every distinct file of the pairs, in order of first use."""
        slot = {}
        for p1, p2, _ in pairs:
            for p in (p1, p2):
                slot.setdefault(p, len(slot))
        return slot

    def _epoch_pairs(self) -> Tuple[np.ndarray, np.ndarray]:
        """(slots (n, 2) int32, labels (n,) float32) of the pairs one epoch runs over."""
        return self._slots, self._labels

    def __len__(self) -> int:
        n = len(self._epoch_pairs()[1])
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        dev = self.device
        epoch, self.epoch = self.epoch, self.epoch + 1
        slots, labels = self._epoch_pairs()
        batches, draws = plan_pair_epoch(len(labels), self.batch_size, self.shuffle, self.drop_last, self.augment)
        if not batches:
            return
        # rows of one batch of m pairs: its m first images, then its m second images (x1's rows first)
        starts = np.cumsum([0] + [len(b) for b in batches])
        order = np.concatenate([np.asarray(b, np.int64) for b in batches])
        rows = np.concatenate([np.concatenate([2 * np.arange(s, e), 2 * np.arange(s, e) + 1]) for s, e in zip(starts[:-1], starts[1:])])
        index_dev = torch.from_numpy(np.ascontiguousarray(slots[order].reshape(-1)[rows])).to(dev)
        labels_dev = torch.from_numpy(labels[order]).to(dev)
        prm_dev = tab_dev = None
        if draws is not None:
            prm, tab = build_pair_params(*(draws[k].reshape(-1)[rows] for k in ("angle", "tx", "ty", "scale", "flip")))
            prm_dev, tab_dev = torch.from_numpy(prm).to(dev), torch.from_numpy(tab).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for s, e in zip(starts[:-1], starts[1:]):
            m, o = int(e - s), 2 * int(s)
            out = torch.empty(2 * m, SIZE, SIZE, dtype=torch.uint8, device=dev)
            self._check(self.lib.siggan_pairs_augment(
                dev.index, self.cache.data_ptr(), self.cache.shape[0], index_dev.data_ptr() + 4 * o,
                prm_dev.data_ptr() + 32 * o if prm_dev is not None else None,
                tab_dev.data_ptr() + 4 * SIZE * o if tab_dev is not None else None,
                out.data_ptr(), 2 * m, SIZE, FILL, stream))
            if self.elastic is not None and self.augment:
                out = warp_u8(out, self.elastic, self.elastic_seed, draw_ids=[(epoch << 32) + o + r for r in range(2 * m)])
            yield out[:m], out[m:], labels_dev[int(s):int(e)]
