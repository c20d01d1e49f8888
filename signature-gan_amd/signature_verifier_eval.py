"""Signature verification model evaluation on the MI355X HIP path.

Drop-in for the reference's ``signature_verifier_eval`` module: the Siamese CNN (``CNNEncoder`` / ``SiameseNetwork``,
reference :39-179) with the reference's attribute names, ``state_dict()`` and checkpoint dictionary, its test dataset and
pair generation, its metrics, report and CLI.  The eval-mode forward runs in HIP (include/siggan_verifier.h,
csrc/verifier.hip); the modules here only hold the parameters.  There is no PyTorch fallback: a forward in training mode
or on CPU tensors raises.  Training the verifier is not part of this package.

Beyond the reference: ``embed_u8`` / ``score_u8`` take uint8 (N, 64, 64) images (what ``Engine.g_generate_u8`` writes and
what a PNG holds) and normalise them on load exactly as ToTensor + Normalize([0.5], [0.5]) would; ``compare`` scores
embeddings that were computed earlier (one query against an enrolled gallery).  ``score_matrix`` / ``pair_counts`` /
``best_matches`` run the pair head over EVERY (query, reference) pair in one HIP call (include/siggan_verifier_pairs.h), and
``evaluate_all_pairs`` / ``--all_pairs`` evaluate a test directory on all N (N - 1) / 2 pairs instead of a sample.
``pair_topk`` takes per-row lists out of the same pass (include/siggan_verifier_topk.h): each row's k highest-scoring
impostors and k lowest- or highest-scoring genuine partners, which is what the trainer's hard-pair mining runs on.
``embed_resized`` / ``input_grad_resized`` take images of another size (the 128x128 Generator's) and shrink them to 64x64 on
the device with Pillow's antialiased bilinear filter (resize.py), as the reference's transform shrinks a file.

The metrics are numpy only (this package imports neither scikit-learn nor matplotlib at module level); the ROC points are
those of ``sklearn.metrics.roc_curve`` with its defaults.  The plots are written when matplotlib can be imported.
"""
import argparse
import ctypes as C
import json
from datetime import datetime
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
from PIL import Image
from torch.utils.data import DataLoader, Dataset

from . import _lib
from . import resize as _resize

IMAGE_SIZE = 64
DEFAULT_MAX_IMAGES = 512
_NO_CPU = "runs on the MI355X HIP path only: move the model and its inputs to a ROCm device (.to('cuda')); there is no CPU path"


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


# =============================================================================
# HIP context
# =============================================================================


class _Context:
    """One siggan_verifier handle: the packed weights and the workspace for up to ``max_images`` images per call."""

    def __init__(self, device, embedding_dim, max_images):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.E, self.max_images = int(embedding_dim), int(max_images)
        h = C.c_void_p()
        _lib.check(self.lib.siggan_verifier_create(self.device.index, self.E, self.max_images, C.byref(h)))
        self._h = h
        self._grad_enabled = False
        self._pairs_rows = 0
        self._topk = (0, 0)                                 # (max_queries, max_k) of siggan_verifier_pairs_topk_enable

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def bind(self, tensors, bn_eps):
        """tensors: the 26 fp32 device tensors in _lib.VERIFIER_WEIGHT_FIELDS order (copied / packed by the library)."""
        w = _lib.VerifierWeights()
        keep = []
        for name, t in zip(_lib.VERIFIER_WEIGHT_FIELDS, tensors):
            t = t.detach()
            if t.device != self.device or t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32 on {self.device}, got {t.dtype} on {t.device}")
            t = t.contiguous()
            keep.append(t)
            setattr(w, name, t.data_ptr())
        w.bn_eps = float(bn_eps)
        _lib.check(self.lib.siggan_verifier_bind(self._h, C.byref(w), self._stream()))

    def _images(self, x, what):
        """-> (contiguous tensor, fmt, n)"""
        if x.device != self.device:
            raise ValueError(f"{what} must live on {self.device}, got {x.device}")
        if x.dim() == 4 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 3 or x.shape[1] != IMAGE_SIZE or x.shape[2] != IMAGE_SIZE:
            raise ValueError(f"{what} must be (N, 1, {IMAGE_SIZE}, {IMAGE_SIZE}) or (N, {IMAGE_SIZE}, {IMAGE_SIZE}), got {tuple(x.shape)}")
        if x.dtype == torch.uint8:
            fmt = _lib.VFMT_U8
        elif x.dtype == torch.float32:
            fmt = _lib.VFMT_F32
        else:
            raise ValueError(f"{what} must be float32 or uint8, got {x.dtype}")
        return x.contiguous(), fmt, x.shape[0]

    def embed(self, x):
        x, fmt, n = self._images(x, "x")
        out = torch.empty(n, self.E, dtype=torch.float32, device=self.device)
        for i in range(0, n, self.max_images):
            c = x[i:i + self.max_images]
            _lib.check(self.lib.siggan_verifier_embed(self._h, _ptr(c), fmt, c.shape[0], _ptr(out[i:]), self._stream()))
        return out

    def score(self, x1, x2):
        x1, fmt, n = self._images(x1, "x1")
        x2, fmt2, n2 = self._images(x2, "x2")
        if fmt != fmt2 or n != n2:
            raise ValueError("x1 and x2 must have the same dtype and batch size")
        if self.max_images < 2:
            raise ValueError("scoring pairs needs a context of at least 2 images")
        e1 = torch.empty(n, self.E, dtype=torch.float32, device=self.device)
        e2 = torch.empty_like(e1)
        s = torch.empty(n, 1, dtype=torch.float32, device=self.device)
        step = self.max_images // 2
        for i in range(0, n, step):
            a, b = x1[i:i + step], x2[i:i + step]
            _lib.check(self.lib.siggan_verifier_score(self._h, _ptr(a), _ptr(b), fmt, a.shape[0], _ptr(e1[i:]), _ptr(e2[i:]),
                                                      _ptr(s[i:]), self._stream()))
        return e1, e2, s

    def compare(self, e1, e2):
        for e in (e1, e2):
            if e.device != self.device or e.dtype != torch.float32 or e.dim() != 2 or e.shape[1] != self.E:
                raise ValueError(f"embeddings must be float32 (N, {self.E}) on {self.device}")
        if e1.shape != e2.shape:
            raise ValueError("e1 and e2 must have the same shape")
        e1, e2 = e1.contiguous(), e2.contiguous()
        s = torch.empty(e1.shape[0], 1, dtype=torch.float32, device=self.device)
        if e1.shape[0]:
            _lib.check(self.lib.siggan_verifier_compare(self._h, _ptr(e1), _ptr(e2), e1.shape[0], _ptr(s), self._stream()))
        return s

    def pairs(self, e_q, ids_q, e_r, ids_r, same_set=False, want_matrix=False, thresholds=None, want_best=False):
        """siggan_verifier_pairs: the head over every pair (q_i, r_j) in one pass.  Returns a dict with the requested groups:
        'score' (nq, nr); 'thresholds' (T,) fp32, 'genuine_counts', 'impostor_counts' (T + 1,) int64; 'best_genuine',
        'best_impostor' (nq,) fp32 with 'best_genuine_index', 'best_impostor_index' (nq,) int32.  ``thresholds``: a host
        sequence / array (or tensor, read back once) of ascending values; that they ascend is checked here, on the host.
        Refusals are ValueError before anything is allocated."""
        nq, nr, thr = check_pairs_args(e_q, ids_q, e_r, ids_r, same_set, want_matrix, thresholds, want_best, self.E, self.device)
        if self._pairs_rows < nq:
            _lib.check(self.lib.siggan_verifier_pairs_enable(self._h, nq))
            self._pairs_rows = nq
        e_q, e_r = e_q.contiguous(), e_r.contiguous()
        ids_q = ids_q.contiguous() if ids_q is not None else None
        ids_r = ids_r.contiguous() if ids_r is not None else None
        new = lambda n, dt: torch.empty(n, dtype=dt, device=self.device)
        res, o = {}, _lib.PairOutputs()
        if want_matrix:
            res["score"] = torch.empty(nq, nr, dtype=torch.float32, device=self.device)
            o.score_dev = res["score"].data_ptr()
        if thr is not None:
            res["thresholds"] = torch.from_numpy(thr).to(self.device)
            res["genuine_counts"], res["impostor_counts"] = new(thr.size + 1, torch.int64), new(thr.size + 1, torch.int64)
            o.threshold_dev, o.n_thresholds = res["thresholds"].data_ptr(), int(thr.size)
            o.genuine_count_dev, o.impostor_count_dev = res["genuine_counts"].data_ptr(), res["impostor_counts"].data_ptr()
        if want_best:
            for k, f, dt in (("best_genuine", "best_genuine_dev", torch.float32), ("best_genuine_index", "best_genuine_index_dev", torch.int32),
                             ("best_impostor", "best_impostor_dev", torch.float32), ("best_impostor_index", "best_impostor_index_dev", torch.int32)):
                res[k] = new(nq, dt)
                setattr(o, f, res[k].data_ptr())
        _lib.check(self.lib.siggan_verifier_pairs(self._h, _ptr(e_q), _ptr(ids_q), nq, _ptr(e_r), _ptr(ids_r), nr, int(bool(same_set)),
                                                  C.byref(o), self._stream()))
        return res

    def pair_topk(self, e_q, ids_q, e_r, ids_r, k, same_set, genuine_lowest, want):
        """siggan_verifier_pairs_topk on one chunk of queries (nq <= PAIR_TOPK_CHUNK is the caller's business): a dict of
        (nq, k) tensors, '<class>_score' fp32 and '<class>_index' int32 for every class in ``want``."""
        nq, nr = e_q.shape[0], e_r.shape[0]
        if self._pairs_rows < 1:
            _lib.check(self.lib.siggan_verifier_pairs_enable(self._h, 1))            # the weight pack; the lists have their own slots
            self._pairs_rows = 1
        rows, kmax = self._topk
        if rows < nq or kmax < k:
            _lib.check(self.lib.siggan_verifier_pairs_topk_enable(self._h, max(rows, nq), max(kmax, k)))
            self._topk = (max(rows, nq), max(kmax, k))
        e_q, e_r = e_q.contiguous(), e_r.contiguous()
        ids_q = ids_q.contiguous() if ids_q is not None else None
        ids_r = ids_r.contiguous() if ids_r is not None else None
        res, o = {}, _lib.PairTopk()
        for c in want:
            res[f"{c}_score"] = torch.empty(nq, k, dtype=torch.float32, device=self.device)
            res[f"{c}_index"] = torch.empty(nq, k, dtype=torch.int32, device=self.device)
            setattr(o, f"{c}_score_dev", res[f"{c}_score"].data_ptr())
            setattr(o, f"{c}_index_dev", res[f"{c}_index"].data_ptr())
        _lib.check(self.lib.siggan_verifier_pairs_topk(self._h, _ptr(e_q), _ptr(ids_q), nq, _ptr(e_r), _ptr(ids_r), nr, int(bool(same_set)),
                                                       int(k), int(bool(genuine_lowest)), C.byref(o), self._stream()))
        return res

    def input_grad(self, x, ref_emb, embed_weight, score_weight, want_terms, want_score, want_emb, dx_out, objective_out):
        if not self._grad_enabled:                         # lazily: contexts that never ask for a gradient pay nothing
            _lib.check(self.lib.siggan_verifier_input_grad_enable(self._h))
            self._grad_enabled = True
        n = x.shape[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self.device)
        dx = dx_out if dx_out is not None else new(n, 1, IMAGE_SIZE, IMAGE_SIZE)
        obj = objective_out if objective_out is not None else new(n)
        terms = new(2, n) if want_terms else None
        score = new(n) if want_score else None
        emb = new(n, self.E) if want_emb else None
        w = _lib.VerifierIdentity(embed_weight, score_weight)
        _lib.check(self.lib.siggan_verifier_input_grad(self._h, _ptr(x), _ptr(ref_emb), n, C.byref(w), _ptr(dx), _ptr(obj), _ptr(terms),
                                                       _ptr(score), _ptr(emb), self._stream()))
        return (dx, obj) + tuple(t for t in (terms, score, emb) if t is not None)

    def input_grad_debug(self, name, shape, dtype=torch.uint8):
        """'route1|2|3' (NCHW), 'fc1_mask', 'cls_mask' uint8, 'diff_sign' int8 of the last input_grad call (test hook)."""
        n = int(np.prod(shape))
        out = torch.empty(n, dtype=dtype, device=self.device)
        _lib.check(self.lib.siggan_verifier_input_grad_debug(self._h, name.encode(), _ptr(out), n, self._stream()))
        return out.view(*shape)

    def debug_tensor(self, name, shape):
        """Stage 'pool1' | 'pool2' | 'pool3' | 'fc1' of the last call in torch's layout (test hook)."""
        n = int(np.prod(shape))
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.siggan_verifier_debug_tensor(self._h, name.encode(), _ptr(out), n, self._stream()))
        return out.view(*shape)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.siggan_verifier_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # interpreter shutdown
            pass


def check_pairs_args(e_q, ids_q, e_r, ids_r, same_set, want_matrix, thresholds, want_best, embedding_dim, device=None):
    """The refusals of siggan_verifier_pairs that can be decided on the host, raised as ValueError before anything is allocated;
    returns (nq, nr, thresholds as an ascending float32 numpy array or None)."""
    if embedding_dim > _lib.PAIR_MAX_DIM:
        raise ValueError(f"all-pairs scoring takes embedding_dim <= {_lib.PAIR_MAX_DIM}, got {embedding_dim}")
    for e, what in ((e_q, "e_q"), (e_r, "e_r")):
        if not isinstance(e, torch.Tensor) or e.dtype != torch.float32 or e.dim() != 2 or e.shape[1] != embedding_dim:
            raise ValueError(f"{what} must be a float32 (N, {embedding_dim}) tensor")
        if e.shape[0] < 1:
            raise ValueError(f"{what} has no rows")
        if device is not None and e.device != device:
            raise ValueError(f"{what} must live on {device}, got {e.device}")
    nq, nr = e_q.shape[0], e_r.shape[0]
    if nq * nr >= 2 ** 62:
        raise ValueError("nq * nr >= 2^62")
    for ids, n, what in ((ids_q, nq, "ids_q"), (ids_r, nr, "ids_r")):
        if ids is not None and (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or tuple(ids.shape) != (n,)
                                or ids.device != e_q.device):
            raise ValueError(f"{what} must be an int32 ({n},) tensor on the embeddings' device, or None")
    if same_set and nq != nr:
        raise ValueError(f"same_set needs the same rows on both sides, got nq = {nq} and nr = {nr}")
    if not (want_matrix or want_best or thresholds is not None):
        raise ValueError("no output requested: ask for the matrix, the counts (thresholds) or the best matches")
    thr = None
    if thresholds is not None:
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().numpy()
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        if not 1 <= thr.size <= _lib.PAIR_MAX_THRESHOLDS:
            raise ValueError(f"the thresholds must hold 1 .. {_lib.PAIR_MAX_THRESHOLDS} values, got {thr.size}")
        if not np.all(np.isfinite(thr)) or np.any(np.diff(thr) < 0):
            raise ValueError("the thresholds must be finite and ascending")
    return nq, nr, thr


PAIR_TOPK_CLASSES = ("impostor", "genuine")
PAIR_TOPK_CHUNK = 4096                      # query rows per siggan_verifier_pairs_topk call: bounds the key slots (32 MiB at k = 16)


def check_pair_topk_args(e_q, ids_q, e_r, ids_r, k, same_set, want, embedding_dim, device=None):
    """The refusals of siggan_verifier_pairs_topk that can be decided on the host, raised as ValueError before anything is
    allocated; returns (nq, nr, the wanted classes in PAIR_TOPK_CLASSES order)."""
    nq, nr, _ = check_pairs_args(e_q, ids_q, e_r, ids_r, same_set, True, None, False, embedding_dim, device)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _lib.PAIR_TOPK_MAX:
        raise ValueError(f"k must be an integer in 1 .. {_lib.PAIR_TOPK_MAX}, got {k!r}")
    if isinstance(want, str):
        want = (want,)
    want = tuple(want)
    if not want or any(c not in PAIR_TOPK_CLASSES for c in want):
        raise ValueError(f"want must name at least one of {PAIR_TOPK_CLASSES}, got {want!r}")
    return nq, nr, tuple(c for c in PAIR_TOPK_CLASSES if c in want)


def _merge_topk(parts, k, lowest):
    """Lists of the same query rows over disjoint reference ranges -> the list over their union: parts is a sequence of
    (score (n, k), index (n, k)) already holding rows of the whole reference set.  Two stable sorts give the kernel's total
    order (score, then row ascending); padding sorts last."""
    score, index = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    none = index < 0
    o = torch.sort(torch.where(none, torch.iinfo(torch.int32).max, index), dim=1, stable=True).indices
    score, index, none = score.gather(1, o), index.gather(1, o), none.gather(1, o)
    o = torch.sort(torch.where(none, float("inf") if lowest else float("-inf"), score), dim=1, stable=True, descending=not lowest).indices
    return score.gather(1, o)[:, :k].contiguous(), index.gather(1, o)[:, :k].contiguous()


def check_identity_weights(embed_weight, score_weight):
    """The refusals of siggan_verifier_input_grad's weights, raised as ValueError before anything is allocated."""
    import math
    w = (float(embed_weight), float(score_weight))
    if any(not math.isfinite(v) or v < 0.0 for v in w):
        raise ValueError(f"the identity weights must be finite and >= 0, got {w}")
    if w == (0.0, 0.0):
        raise ValueError("both identity weights are 0")
    return w


def check_input_grad_shapes(x, ref_emb, embedding_dim, max_images, dx_out=None, objective_out=None):
    """Shape / dtype refusals of input_grad (host only); returns N."""
    for t, what in ((x, "x"), (ref_emb, "ref_emb")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{what} must be a float32 tensor")
    if not ((x.dim() == 4 and tuple(x.shape[1:]) == (1, IMAGE_SIZE, IMAGE_SIZE))
            or (x.dim() == 3 and tuple(x.shape[1:]) == (IMAGE_SIZE, IMAGE_SIZE))):
        raise ValueError(f"x must be (N, 1, {IMAGE_SIZE}, {IMAGE_SIZE}), got {tuple(x.shape)}")
    n = x.shape[0]
    if not 1 <= n <= max_images:
        raise ValueError(f"input_grad takes 1 .. max_images = {max_images} images per call, got {n}")
    if tuple(ref_emb.shape) != (n, embedding_dim):
        raise ValueError(f"ref_emb must be ({n}, {embedding_dim}), got {tuple(ref_emb.shape)}")
    for t, shape, what in ((dx_out, (n, 1, IMAGE_SIZE, IMAGE_SIZE), "dx_out"), (objective_out, (n,), "objective_out")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != int(np.prod(shape))):
            raise ValueError(f"{what} must be float32 with {int(np.prod(shape))} elements")
    return n


class _HipModule(nn.Module):
    """Shared plumbing: a lazily created context whose packs are refreshed after the weights change."""

    def _init_hip(self, max_images):
        self.max_images = int(max_images)
        self._ctx = None
        self._stale = True

    def params_changed(self):
        """Tell the HIP path that parameters or buffers were written in place (the packs are rebuilt on the next call)."""
        self._stale = True
        for m in self.children():
            if isinstance(m, _HipModule):
                m.params_changed()

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        if self._ctx is not None:
            self._ctx.close()
        self._ctx, self._stale = None, True
        return out

    def load_state_dict(self, state_dict, strict=True, assign=False):
        out = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self.params_changed()
        return out

    def _weights(self):
        raise NotImplementedError

    def _context(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} {_NO_CPU}")
        if self._ctx is None or self._ctx.max_images != self.max_images:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = _Context(dev, self.embedding_dim, self.max_images)
            self._stale = True
        if self._stale:
            tensors, eps = self._weights()
            self._ctx.bind(tensors, eps)
            self._stale = False
        return self._ctx

    def _on_device(self, *xs):
        if self.training:
            raise RuntimeError(f"{type(self).__name__}: only the eval-mode forward is built (call .eval()); "
                               "training the verifier is not part of this package")
        for x in xs:
            if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
                raise RuntimeError(f"{type(self).__name__} {_NO_CPU}")


# =============================================================================
# Model Architecture (must match training)
# =============================================================================


class CNNEncoder(_HipModule):
    """
    CNN encoder for extracting features from 64x64 signature images.

    Architecture:
        Conv2d(1,32) -> Conv2d(32,64) -> Conv2d(64,128) -> FC -> embedding
    """

    def __init__(self, embedding_dim: int = 128, max_images: int = DEFAULT_MAX_IMAGES) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=5, stride=1, padding=2)
        self.bn1 = nn.BatchNorm2d(32)
        self.pool1 = nn.MaxPool2d(kernel_size=2, stride=2)

        self.conv2 = nn.Conv2d(32, 64, kernel_size=5, stride=1, padding=2)
        self.bn2 = nn.BatchNorm2d(64)
        self.pool2 = nn.MaxPool2d(kernel_size=2, stride=2)

        self.conv3 = nn.Conv2d(64, 128, kernel_size=3, stride=1, padding=1)
        self.bn3 = nn.BatchNorm2d(128)
        self.pool3 = nn.MaxPool2d(kernel_size=2, stride=2)

        # After 3 pooling layers: 64 -> 32 -> 16 -> 8
        self.fc1 = nn.Linear(128 * 8 * 8, 512)
        self.dropout = nn.Dropout(0.5)
        self.fc2 = nn.Linear(512, embedding_dim)
        self.embedding_dim = int(embedding_dim)
        self._init_hip(max_images)

    def _encoder_tensors(self):
        out = []
        for conv, bn in ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)):
            out += [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        out += [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias]
        if not (self.bn1.eps == self.bn2.eps == self.bn3.eps):
            raise ValueError("the three BatchNorm layers must share one eps")
        return out, self.bn1.eps

    def _weights(self):
        enc, eps = self._encoder_tensors()
        dev, e = self.fc2.weight.device, self.embedding_dim
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)   # a bare encoder has no pair head
        return enc + [z(64, e), z(64), z(1, 64), z(1)], eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """(batch_size, 1, 64, 64) in [-1, 1] -> L2-normalised (batch_size, embedding_dim)."""
        self._on_device(x)
        return self._context().embed(x)

    def embed_u8(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 (N, 64, 64) -> embeddings; bit-identical to forward() on ((b / 255) - 0.5) / 0.5."""
        self._on_device(images)
        if images.dtype != torch.uint8:
            raise ValueError(f"embed_u8 takes uint8 images, got {images.dtype}")
        return self._context().embed(images)


class SiameseNetwork(_HipModule):
    """
    Siamese Network for signature verification.

    Uses twin CNN encoders with shared weights to compare two signatures
    and determine if they belong to the same person.
    """

    def __init__(self, embedding_dim: int = 128, max_images: int = DEFAULT_MAX_IMAGES) -> None:
        super().__init__()
        self.encoder = CNNEncoder(embedding_dim=embedding_dim, max_images=max_images)
        self.embedding_dim = embedding_dim

        # Classifier for BCE loss approach
        self.classifier = nn.Sequential(
            nn.Linear(embedding_dim, 64),
            nn.ReLU(),
            nn.Dropout(0.3),
            nn.Linear(64, 1),
            nn.Sigmoid()
        )
        self._init_hip(max_images)

    def _weights(self):
        enc, eps = self.encoder._encoder_tensors()
        c0, c3 = self.classifier[0], self.classifier[3]
        return enc + [c0.weight, c0.bias, c3.weight, c3.bias], eps

    def forward_one(self, x: torch.Tensor) -> torch.Tensor:
        """Embedding of a batch of images (one encoder pass)."""
        self._on_device(x)
        return self._context().embed(x)

    def forward(self, x1: torch.Tensor, x2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(embedding1, embedding2, similarity (B, 1)); both images of every pair go through the encoder as one batch.
        Batches larger than the context (``max_images`` images, i.e. max_images // 2 pairs) are chunked."""
        self._on_device(x1, x2)
        return self._context().score(x1, x2)

    def embed_u8(self, images: torch.Tensor) -> torch.Tensor:
        self._on_device(images)
        if images.dtype != torch.uint8:
            raise ValueError(f"embed_u8 takes uint8 images, got {images.dtype}")
        return self._context().embed(images)

    def score_u8(self, images1: torch.Tensor, images2: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """forward() on uint8 (B, 64, 64) images, normalised on load."""
        self._on_device(images1, images2)
        if images1.dtype != torch.uint8 or images2.dtype != torch.uint8:
            raise ValueError("score_u8 takes uint8 images")
        return self._context().score(images1, images2)

    def compare(self, e1: torch.Tensor, e2: torch.Tensor) -> torch.Tensor:
        """Similarity (B, 1) of embeddings computed earlier (forward_one / embed_u8)."""
        self._on_device(e1, e2)
        return self._context().compare(e1, e2)

    def pairs(self, e_q: torch.Tensor, ids_q: Optional[torch.Tensor], e_r: torch.Tensor, ids_r: Optional[torch.Tensor],
              same_set: bool = False, want_matrix: bool = False, thresholds=None, want_best: bool = False) -> Dict[str, torch.Tensor]:
        """The pair head over every (query, reference) pair of two embedding sets in ONE HIP call (see _Context.pairs): any
        of the score matrix, the per-class threshold histograms and each query row's best genuine / impostor match.  A pair is
        genuine when its int32 ids agree; without ids every pair counts as impostor.  ``same_set``: both sides are the same
        rows -- counts cover j > i, a row is never its own match.  score[i, j] is compare(e_q[i], e_r[j]) bit for bit."""
        check_pairs_args(e_q, ids_q, e_r, ids_r, same_set, want_matrix, thresholds, want_best, self.embedding_dim)
        self._on_device(e_q, e_r)
        return self._context().pairs(e_q, ids_q, e_r, ids_r, same_set, want_matrix, thresholds, want_best)

    def score_matrix(self, e_q: torch.Tensor, e_r: torch.Tensor) -> torch.Tensor:
        """Similarity (nq, nr) of every query embedding against every reference embedding."""
        return self.pairs(e_q, None, e_r, None, want_matrix=True)["score"]

    def pair_counts(self, e: torch.Tensor, ids: Optional[torch.Tensor], thresholds, other: Optional[torch.Tensor] = None,
                    other_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(genuine_counts, impostor_counts), int64 (T + 1,): bin b counts the pairs with t[b-1] <= score < t[b].  Without
        ``other`` the pairs are the N (N - 1) / 2 unordered pairs of ``e``; with it, every (e_i, other_j)."""
        if other is None:
            out = self.pairs(e, ids, e, ids, same_set=True, thresholds=thresholds)
        else:
            out = self.pairs(e, ids, other, other_ids, thresholds=thresholds)
        return out["genuine_counts"], out["impostor_counts"]

    def best_matches(self, e_q: torch.Tensor, ids_q: Optional[torch.Tensor], e_r: torch.Tensor, ids_r: Optional[torch.Tensor],
                     same_set: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(best_genuine, best_genuine_index, best_impostor, best_impostor_index) per query row: the highest score among the
        genuine / impostor references and its row (the lower row on equal scores); -1.0 and -1 where a row has none."""
        out = self.pairs(e_q, ids_q, e_r, ids_r, same_set=same_set, want_best=True)
        return out["best_genuine"], out["best_genuine_index"], out["best_impostor"], out["best_impostor_index"]

    def pair_topk(self, e_q: torch.Tensor, ids_q: Optional[torch.Tensor], e_r: torch.Tensor, ids_r: Optional[torch.Tensor], k: int,
                  same_set: bool = False, genuine_lowest: bool = True, want=PAIR_TOPK_CLASSES) -> Dict[str, torch.Tensor]:
        """Per query row the ``k`` (1 .. 16) highest-scoring impostor references and the ``k`` lowest-scoring (``genuine_lowest``,
        the hard ones) or highest-scoring genuine references, out of the all-pairs pass in HIP (include/siggan_verifier_topk.h):
        {'impostor_score', 'impostor_index', 'genuine_score', 'genuine_index'} (those of the classes in ``want``), each (nq, k),
        fp32 scores that are ``score_matrix``'s bit for bit and int32 rows of ``e_r``.  Highest lists are ordered by (score
        descending, row ascending), lowest lists by (score ascending, row ascending); positions beyond a row's candidates hold
        -1.0 / -1.  ids, ``same_set``: as in ``pairs``.  The matrix is not formed; queries go through in chunks of
        PAIR_TOPK_CHUNK rows (rows are independent: the chunking does not show in the result).  With ``same_set`` a chunk that
        is not the whole set scores its own rows (same_set), the rows before and the rows after in three calls and merges
        the lists by the same order."""
        nq, nr, want = check_pair_topk_args(e_q, ids_q, e_r, ids_r, k, same_set, want, self.embedding_dim)
        self._on_device(e_q, e_r)
        ctx = self._context()
        check_pair_topk_args(e_q, ids_q, e_r, ids_r, k, same_set, want, self.embedding_dim, ctx.device)
        e_q, e_r = e_q.contiguous(), e_r.contiguous()
        chunk = int(PAIR_TOPK_CHUNK)
        if nq <= chunk:
            return ctx.pair_topk(e_q, ids_q, e_r, ids_r, k, same_set, genuine_lowest, want)
        outs = []
        for a in range(0, nq, chunk):
            b = min(a + chunk, nq)
            q, qi = e_q[a:b], (ids_q[a:b] if ids_q is not None else None)
            if not same_set:
                outs.append(ctx.pair_topk(q, qi, e_r, ids_r, k, False, genuine_lowest, want))
                continue
            parts = []
            for lo, hi, same in ((0, a, False), (a, b, True), (b, nr, False)):
                if hi > lo:
                    o = ctx.pair_topk(q, qi, e_r[lo:hi], ids_r[lo:hi] if ids_r is not None else None, k, same, genuine_lowest, want)
                    parts.append({n: (torch.where(t < 0, t, t + lo) if n.endswith("_index") else t) for n, t in o.items()})
            merged = {}
            for c in want:
                s, i = _merge_topk([(p[f"{c}_score"], p[f"{c}_index"]) for p in parts], k, genuine_lowest and c == "genuine")
                merged[f"{c}_score"], merged[f"{c}_index"] = s, i
            outs.append(merged)
        return {n: torch.cat([o[n] for o in outs]) for n in outs[0]}

    def input_grad(self, x: torch.Tensor, ref_emb: torch.Tensor, embed_weight: float = 1.0, score_weight: float = 0.0,
                   want_terms: bool = False, want_score: bool = False, dx_out: Optional[torch.Tensor] = None,
                   objective_out: Optional[torch.Tensor] = None, want_emb: bool = False):
        """The eval-mode gradient with respect to the images ``x`` (N, 1, 64, 64) fp32 of the per-image identity objective
        embed_weight * 0.5 * |e(x) - r|^2 + score_weight * -max(log s(e(x), r), -100) against the constant reference
        embeddings ``ref_emb`` (N, E) (forward_one / embed_u8 of the targets), in HIP (include/siggan_verifier_grad.h): BatchNorm
        is its running-statistics affine, no dropout, images do not interact.  Returns (dx (N, 1, 64, 64), objective (N,)
        [, terms (2, N) unweighted, 0 where the weight is 0][, score (N,)][, emb (N, E)]).  ``dx_out`` / ``objective_out``:
        caller-owned contiguous fp32 device tensors the results are written into.  At most ``max_images`` images per call.
        Nothing synchronises with the host."""
        we, ws = check_identity_weights(embed_weight, score_weight)
        n = check_input_grad_shapes(x, ref_emb, self.embedding_dim, self.max_images, dx_out, objective_out)
        self._on_device(x, ref_emb)
        ctx = self._context()
        for t, what in ((x, "x"), (ref_emb, "ref_emb"), (dx_out, "dx_out"), (objective_out, "objective_out")):
            if t is not None and (t.device != ctx.device or not t.is_contiguous()):
                raise ValueError(f"{what} must be contiguous on {ctx.device}")
        return ctx.input_grad(x.view(n, 1, IMAGE_SIZE, IMAGE_SIZE), ref_emb, we, ws, want_terms, want_score, want_emb, dx_out,
                              objective_out)

    def embed_resized(self, images: torch.Tensor) -> torch.Tensor:
        """Embeddings of uint8 or fp32 images (N, H, W) / (N, 1, H, W) of any size the resize takes (1 .. 1024 per side), shrunk
        to 64x64 on the device the way the reference's transforms.Resize((64, 64)) shrinks a file (resize.py): bytes by
        resize_u8 -- Pillow's bytes -- then embed_u8, fp32 by resize_f32 then forward_one.  64x64 input goes to those two
        directly: no copy, the same bits."""
        self._on_device(images)
        if images.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"embed_resized takes uint8 or float32 images, got {images.dtype}")
        if tuple(images.shape[-2:]) != (IMAGE_SIZE, IMAGE_SIZE):
            images = (_resize.resize_u8 if images.dtype == torch.uint8 else _resize.resize_f32)(images.contiguous(), IMAGE_SIZE)
        return self._context().embed(images)

    def input_grad_resized(self, x: torch.Tensor, ref_emb: torch.Tensor, embed_weight: float = 1.0, score_weight: float = 0.0,
                           want_terms: bool = False, want_score: bool = False, dx_out: Optional[torch.Tensor] = None,
                           objective_out: Optional[torch.Tensor] = None, want_emb: bool = False):
        """input_grad of the identity objective at resize_f32(x) for fp32 images ``x`` (N, 1, H, W) of any size the resize
        takes, carried back to x: resize_f32 -> input_grad -> resize_f32_adjoint, three HIP calls and nothing else.  Returns
        what input_grad returns with dx (N, 1, H, W); ``dx_out`` is of that size too.  64x64 input is input_grad itself."""
        if not isinstance(x, torch.Tensor) or tuple(x.shape[-2:]) == (IMAGE_SIZE, IMAGE_SIZE):
            return self.input_grad(x, ref_emb, embed_weight, score_weight, want_terms, want_score, dx_out, objective_out, want_emb)
        check_identity_weights(embed_weight, score_weight)
        if x.dtype != torch.float32 or not (x.dim() == 4 and x.shape[1] == 1):
            raise ValueError(f"x must be float32 (N, 1, H, W), got {x.dtype} {tuple(x.shape)}")
        self._on_device(x, ref_emb)
        small = _resize.resize_f32(x, IMAGE_SIZE)
        res = self.input_grad(small, ref_emb, embed_weight, score_weight, want_terms, want_score, None, objective_out, want_emb)
        dx = _resize.resize_f32_adjoint(res[0], tuple(x.shape[-2:]), out=dx_out)
        return (dx.view(x.shape),) + tuple(res[1:])

    def input_grad_debug(self, name, shape, dtype=torch.uint8):
        return self._context().input_grad_debug(name, shape, dtype)

    def debug_tensor(self, name, shape):
        return self._context().debug_tensor(name, shape)


# =============================================================================
# Test Dataset
# =============================================================================


def load_uint8(path: Union[str, Path]) -> np.ndarray:
    """PIL 'L' + bilinear resize to 64x64 (what torchvision's Resize does on a PIL image) -> uint8 (64, 64)."""
    img = Image.open(path).convert('L').resize((IMAGE_SIZE, IMAGE_SIZE), Image.BILINEAR)
    return np.asarray(img, dtype=np.uint8)


def normalize_uint8(a: np.ndarray) -> np.ndarray:
    """ToTensor then Normalize([0.5], [0.5]): two fp32 operations, in this order."""
    v = a.astype(np.float32) / np.float32(255.0)
    return (v - np.float32(0.5)) / np.float32(0.5)


def default_transform(img: Image.Image) -> torch.Tensor:
    """Resize((64, 64)) -> Grayscale(1) -> ToTensor -> Normalize([0.5], [0.5]) with PIL + numpy: (1, 64, 64) fp32."""
    a = np.asarray(img.convert('L').resize((IMAGE_SIZE, IMAGE_SIZE), Image.BILINEAR), dtype=np.uint8)
    return torch.from_numpy(normalize_uint8(a)[None])


class SignatureTestDataset(Dataset):
    """
    Test dataset for signature verification evaluation.

    Supports two directory structures:
        1. Organized by user: test_dir/user_id/*.png
        2. Flat with naming convention: test_dir/userID_sigNum.png

    Generates genuine (same user) and forgery (different user) pairs with the reference's np.random calls.
    ``uint8=True`` hands out the resized uint8 (64, 64) images instead of normalised fp32 (the byte route).
    """

    def __init__(self, test_dir: str, transform=None, pairs_per_user: int = 20, seed: int = 42, uint8: bool = False) -> None:
        self.test_dir = Path(test_dir)
        self.pairs_per_user = pairs_per_user
        self.transform = transform or default_transform
        self.uint8 = bool(uint8)

        np.random.seed(seed)

        self.user_signatures: Dict[str, List[Path]] = {}
        self._load_signatures()

        self.pairs: List[Tuple[Path, Path, int]] = []
        self._generate_pairs()

    def _load_signatures(self) -> None:
        image_extensions = {'.png', '.jpg', '.jpeg', '.bmp', '.tiff'}
        subdirs = [d for d in self.test_dir.iterdir() if d.is_dir()]
        if subdirs:
            for user_dir in subdirs:
                user_id = user_dir.name
                user_images = [f for f in user_dir.iterdir() if f.suffix.lower() in image_extensions]
                if len(user_images) >= 2:
                    self.user_signatures[user_id] = user_images
        else:
            all_images = [f for f in self.test_dir.iterdir() if f.suffix.lower() in image_extensions]
            for img_path in all_images:
                filename = img_path.stem
                parts = filename.split('_')
                user_id = parts[0] if parts else filename
                if user_id not in self.user_signatures:
                    self.user_signatures[user_id] = []
                self.user_signatures[user_id].append(img_path)
            self.user_signatures = {k: v for k, v in self.user_signatures.items() if len(v) >= 2}
        print(f"[Test Dataset] Loaded {len(self.user_signatures)} users")

    def _generate_pairs(self) -> None:
        user_ids = list(self.user_signatures.keys())
        if len(user_ids) < 2:
            print("WARNING: Need at least 2 users to generate forgery pairs")
            return
        for user_id in user_ids:
            user_sigs = self.user_signatures[user_id]
            # genuine pairs (same user), label 1
            num_genuine = min(self.pairs_per_user, len(user_sigs) * (len(user_sigs) - 1) // 2)
            for _ in range(num_genuine):
                if len(user_sigs) >= 2:
                    indices = np.random.choice(len(user_sigs), 2, replace=False)
                    self.pairs.append((user_sigs[indices[0]], user_sigs[indices[1]], 1))
            # forgery pairs (different users), label 0
            other_users = [u for u in user_ids if u != user_id]
            for _ in range(self.pairs_per_user):
                other_user = np.random.choice(other_users)
                sig1 = user_sigs[np.random.randint(len(user_sigs))]
                other_sigs = self.user_signatures[other_user]
                sig2 = other_sigs[np.random.randint(len(other_sigs))]
                self.pairs.append((sig1, sig2, 0))
        np.random.shuffle(self.pairs)
        genuine_count = sum(1 for _, _, label in self.pairs if label == 1)
        forgery_count = len(self.pairs) - genuine_count
        print(f"[Test Dataset] Generated {len(self.pairs)} pairs: "
              f"{genuine_count} genuine, {forgery_count} forgery")

    def __len__(self) -> int:
        return len(self.pairs)

    def get_uint8(self, idx: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The pair as resized uint8 (64, 64) tensors; normalize_uint8 of them is the default transform bit for bit."""
        sig1_path, sig2_path, label = self.pairs[idx]
        return (torch.from_numpy(load_uint8(sig1_path).copy()), torch.from_numpy(load_uint8(sig2_path).copy()),
                torch.tensor(label, dtype=torch.float32))

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if self.uint8:
            return self.get_uint8(idx)
        sig1_path, sig2_path, label = self.pairs[idx]
        img1 = Image.open(sig1_path).convert('L')
        img2 = Image.open(sig2_path).convert('L')
        if self.transform:
            img1 = self.transform(img1)
            img2 = self.transform(img2)
        return img1, img2, torch.tensor(label, dtype=torch.float32)


# =============================================================================
# Model Loading
# =============================================================================


def load_model(checkpoint_path: str, device: torch.device, embedding_dim: Optional[int] = None
               ) -> Tuple[SiameseNetwork, Dict[str, Any]]:
    """Load a trained Siamese model from the reference's checkpoint dictionary; returns (model, metadata)."""
    checkpoint_path = Path(checkpoint_path)
    if not checkpoint_path.exists():
        raise FileNotFoundError(f"Checkpoint not found: {checkpoint_path}")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"load_model: the verifier {_NO_CPU}")

    checkpoint = torch.load(checkpoint_path, map_location=device, weights_only=False)
    emb_dim = embedding_dim or checkpoint.get('embedding_dim', 128)

    model = SiameseNetwork(embedding_dim=emb_dim)
    model.load_state_dict(checkpoint['model_state_dict'])
    model.to(device)
    model.eval()

    metadata = {
        'embedding_dim': emb_dim,
        'val_accuracy': checkpoint.get('val_accuracy', None),
        'epoch': checkpoint.get('epoch', None),
        'includes_synthetic': checkpoint.get('includes_synthetic', False),
        'checkpoint_path': str(checkpoint_path)
    }
    acc = f"{metadata['val_accuracy']:.4f}" if metadata['val_accuracy'] else 'N/A'
    print(f"[Model] Loaded from: {checkpoint_path}")
    print(f"[Model] Embedding dim: {emb_dim}, Val accuracy: {acc}")
    return model, metadata


# =============================================================================
# Metrics Computation (numpy; the points of sklearn.metrics.roc_curve / det_curve)
# =============================================================================


def _binary_clf_curve(y_true: np.ndarray, y_scores: np.ndarray):
    """False / true positive counts at every distinct score, decreasing (positive label 1)."""
    y_true = np.asarray(y_true).ravel() == 1
    y_scores = np.asarray(y_scores, dtype=np.float64).ravel()
    order = np.argsort(y_scores, kind="mergesort")[::-1]
    y_scores, y_true = y_scores[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_scores))[0], y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps, y_scores[idx]


def roc_curve(y_true: np.ndarray, y_scores: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(fpr, tpr, thresholds) as sklearn.metrics.roc_curve with its defaults: collinear intermediate points dropped, a
    leading (0, 0) point at threshold inf; a class with no samples gives NaN rates."""
    return _roc_from_counts(*_binary_clf_curve(y_true, y_scores))


def _roc_from_counts(fps, tps, thr):
    """roc_curve's points from the cumulative false / true positive counts at descending thresholds."""
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    tps, fps, thr = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thr]
    fpr = np.repeat(np.nan, fps.shape) if fps[-1] <= 0 else fps / fps[-1]
    tpr = np.repeat(np.nan, tps.shape) if tps[-1] <= 0 else tps / tps[-1]
    return fpr, tpr, thr


def det_curve(y_true: np.ndarray, y_scores: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(fpr, fnr, thresholds) as sklearn.metrics.det_curve."""
    fps, tps, thr = _binary_clf_curve(y_true, y_scores)
    fns = tps[-1] - tps
    p_count, n_count = tps[-1], fps[-1]
    first = fps.searchsorted(fps[0], side="right") - 1 if fps.searchsorted(fps[0], side="right") > 0 else None
    last = tps.searchsorted(tps[-1]) + 1
    sl = slice(first, last)
    return fps[sl][::-1] / n_count, fns[sl][::-1] / p_count, thr[sl][::-1]


def auc(x: np.ndarray, y: np.ndarray) -> float:
    """Trapezoidal area (x monotonic), as sklearn.metrics.auc."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dx = np.diff(x)
    direction = -1.0 if np.any(dx < 0) and np.all(dx <= 0) else 1.0
    return float(direction * np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def compute_verification_metrics(y_true: np.ndarray, y_scores: np.ndarray, y_pred: np.ndarray, threshold: float = 0.5
                                 ) -> Dict[str, float]:
    """The reference's metrics dictionary (FAR, FRR, EER, ROC-AUC, ...) for labels 1 = genuine, 0 = forgery."""
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    accuracy = np.mean(y_true == y_pred) if y_true.size else float('nan')
    tn = int(np.sum((y_true == 0) & (y_pred == 0)))
    fp = int(np.sum((y_true == 0) & (y_pred == 1)))
    fn = int(np.sum((y_true == 1) & (y_pred == 0)))
    tp = int(np.sum((y_true == 1) & (y_pred == 1)))

    # FAR: forgeries accepted as genuine; FRR: genuine signatures rejected
    total_forgeries = fp + tn
    far = fp / total_forgeries if total_forgeries > 0 else 0.0
    total_genuine = fn + tp
    frr = fn / total_genuine if total_genuine > 0 else 0.0

    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
    specificity = tn / (tn + fp) if (tn + fp) > 0 else 0.0

    fpr, tpr, roc_thresholds = roc_curve(y_true, y_scores)
    roc_auc = auc(fpr, tpr)

    # EER: the ROC point where FAR = FRR (an all-NaN curve, i.e. a class without samples, raises as np.nanargmin does)
    fnr = 1 - tpr
    eer_threshold_idx = np.nanargmin(np.abs(fpr - fnr))
    eer = (fpr[eer_threshold_idx] + fnr[eer_threshold_idx]) / 2
    eer_threshold = roc_thresholds[eer_threshold_idx] if len(roc_thresholds) > eer_threshold_idx else threshold

    return {
        'accuracy': float(accuracy),
        'far': float(far),
        'frr': float(frr),
        'eer': float(eer),
        'eer_threshold': float(eer_threshold),
        'precision': float(precision),
        'recall': float(recall),
        'f1_score': float(f1),
        'specificity': float(specificity),
        'roc_auc': float(roc_auc),
        'true_positives': int(tp),
        'true_negatives': int(tn),
        'false_positives': int(fp),
        'false_negatives': int(fn),
        'total_genuine': int(total_genuine),
        'total_forgeries': int(total_forgeries),
        'threshold': float(threshold)
    }


def compute_eer_from_scores(y_true: np.ndarray, y_scores: np.ndarray) -> Tuple[float, float]:
    """(EER value, EER threshold) from scores."""
    fpr, tpr, thresholds = roc_curve(y_true, y_scores)
    fnr = 1 - tpr
    eer_idx = np.nanargmin(np.abs(fpr - fnr))
    eer = (fpr[eer_idx] + fnr[eer_idx]) / 2
    eer_threshold = thresholds[eer_idx] if len(thresholds) > eer_idx else 0.5
    return float(eer), float(eer_threshold)


# =============================================================================
# Metrics from threshold histograms (the counts of SiameseNetwork.pair_counts)
# =============================================================================


def threshold_as_float32(threshold: float) -> np.float32:
    """The smallest float32 >= threshold: for a float32 score s, s >= threshold (as evaluate_model compares, in float64)
    holds exactly when s >= this value."""
    f = np.float32(threshold)
    if float(f) < float(threshold):
        f = np.nextafter(f, np.float32(np.inf))
    return f


def default_threshold_grid(threshold: float = 0.5) -> np.ndarray:
    """Sorted unique float32 thresholds, at most 4096: k / 1024, the sigmoid of a uniform logit grid on [-16, 16] (resolution
    where saturated scores live) and ``threshold`` itself (as threshold_as_float32)."""
    lin = np.arange(1025, dtype=np.float64) / 1024.0
    logit = np.linspace(-16.0, 16.0, _lib.PAIR_MAX_THRESHOLDS - lin.size - 1)
    grid = np.concatenate([lin, 1.0 / (1.0 + np.exp(-logit))]).astype(np.float32)
    return np.unique(np.concatenate([grid, np.array([threshold_as_float32(threshold)], dtype=np.float32)]))


def metrics_from_counts(thresholds, genuine_counts, impostor_counts, threshold: float = 0.5) -> Dict[str, Any]:
    """compute_verification_metrics' dictionary from per-class histograms over an ascending float32 threshold grid (bin b of
    T + 1 counts the pairs with t[b-1] <= score < t[b]) instead of from the scores.

    The confusion matrix at ``threshold`` is exact; threshold_as_float32(threshold) must be one of the grid's values
    (default_threshold_grid puts it there), else ValueError.  The ROC points are the exact points of the true curve at the
    grid's thresholds, ``roc_auc`` is their trapezoid and ``eer`` / ``eer_threshold`` come from them as in
    compute_verification_metrics; with every distinct score in the grid all of these are the true values.

    Two more keys say how far a coarser grid can be off.  Between two exact points the true (monotone) curve cannot leave the
    rectangle they span: ``roc_auc_bounds`` sums the rectangles' lower and upper areas, and ``eer_bounds`` is the range of
    (FAR + FRR) / 2 over the stretch of curve in which the reference's EER point must lie (from the last provable corner before
    the FAR = FRR crossing to the first one after it; roc_curve drops interior points of straight runs, so the point can sit
    at the end of a run).  A bin that spans a single float32 value holds tied scores only, so nothing is unknown inside it:
    when that is true of every occupied bin, both brackets collapse onto the value."""
    t = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    g = np.asarray(genuine_counts, dtype=np.int64).reshape(-1)
    im = np.asarray(impostor_counts, dtype=np.int64).reshape(-1)
    if t.size < 1 or g.size != t.size + 1 or im.size != t.size + 1 or np.any(np.diff(t) < 0):
        raise ValueError("metrics_from_counts takes T ascending thresholds and two arrays of T + 1 counts")
    k = int(np.searchsorted(t, threshold_as_float32(threshold), side="left"))
    if k >= t.size or t[k] != threshold_as_float32(threshold):
        raise ValueError(f"threshold {threshold} is not one of the grid's values: the confusion matrix would not be exact")
    total_genuine, total_forgeries = int(g.sum()), int(im.sum())
    # pairs with score >= t[b], per class: everything in bins b + 1 .. T
    tp_at = np.cumsum(g[::-1])[::-1][1:]
    fp_at = np.cumsum(im[::-1])[::-1][1:]
    tp, fp = int(tp_at[k]), int(fp_at[k])
    fn, tn = total_genuine - tp, total_forgeries - fp
    n = total_genuine + total_forgeries
    accuracy = (tp + tn) / n if n else float('nan')
    far = fp / total_forgeries if total_forgeries > 0 else 0.0
    frr = fn / total_genuine if total_genuine > 0 else 0.0
    precision = tp / (tp + fp) if (tp + fp) > 0 else 0.0
    recall = tp / (tp + fn) if (tp + fn) > 0 else 0.0
    f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0.0
    specificity = tn / (tn + fp) if (tn + fp) > 0 else 0.0

    # the curve's distinct exact points, thresholds descending: grid value b gives a new point when bin b + 1 is occupied;
    # scores below the lowest grid value (bin 0) add the end point at threshold -inf
    occupied = (g + im) > 0
    keep = np.where(occupied[1:])[0][::-1]
    fps, tps, thr = fp_at[keep].astype(np.float64), tp_at[keep].astype(np.float64), t[keep].astype(np.float64)
    if occupied[0]:
        fps, tps, thr = np.r_[fps, float(total_forgeries)], np.r_[tps, float(total_genuine)], np.r_[thr, -np.inf]
    if fps.size == 0:
        raise ValueError("metrics_from_counts: the counts are all zero")
    fpr, tpr, roc_thresholds = _roc_from_counts(fps, tps, thr)
    roc_auc = auc(fpr, tpr)
    fnr = 1 - tpr
    eer_idx = np.nanargmin(np.abs(fpr - fnr))
    eer = (fpr[eer_idx] + fnr[eer_idx]) / 2
    eer_threshold = roc_thresholds[eer_idx] if len(roc_thresholds) > eer_idx else threshold

    # brackets, on every exact point (nothing dropped), (0, 0) first
    x = np.r_[0.0, fps] / total_forgeries if total_forgeries > 0 else np.full(fps.size + 1, np.nan)
    y = np.r_[0.0, tps] / total_genuine if total_genuine > 0 else np.full(tps.size + 1, np.nan)
    upper_edge = np.r_[t[1:], np.float32(np.inf)]
    single = np.r_[False, np.nextafter(t, np.float32(np.inf)) == upper_edge]          # per bin: one float32 value only
    exact = bool(np.all(single[occupied]))
    if exact or not (total_forgeries > 0 and total_genuine > 0):
        auc_bounds, eer_bounds = (roc_auc, roc_auc), (float(eer), float(eer))
    else:
        dx = np.diff(x)
        auc_bounds = (float(np.sum(dx * y[:-1])), float(np.sum(dx * y[1:])))
        cx, cy = np.r_[0.0, fps], np.r_[0.0, tps]                                     # counts: exact collinearity tests
        d = cx * total_genuine + cy * total_forgeries - float(total_genuine) * total_forgeries
        ia, ib = int(np.where(d <= 0)[0][-1]), int(np.where(d >= 0)[0][0])
        last = cx.size - 1

        def straight(i):                                                               # points i - 1, i, i + 1 on one line
            if i < 1 or i > last - 1:
                return False
            return (cx[i] - cx[i - 1]) * (cy[i + 1] - cy[i]) == (cy[i] - cy[i - 1]) * (cx[i + 1] - cx[i])
        lo = ia - 2
        while lo > 0 and straight(lo + 1):
            lo -= 1
        hi = ib + 2
        while hi < last and straight(hi - 1):
            hi += 1
        lo, hi = max(lo, 0), min(hi, last)
        eer_bounds = (float((x[lo] + 1 - y[hi]) / 2), float((x[hi] + 1 - y[lo]) / 2))

    return {
        'accuracy': float(accuracy), 'far': float(far), 'frr': float(frr), 'eer': float(eer), 'eer_threshold': float(eer_threshold),
        'precision': float(precision), 'recall': float(recall), 'f1_score': float(f1), 'specificity': float(specificity),
        'roc_auc': float(roc_auc), 'true_positives': tp, 'true_negatives': tn, 'false_positives': fp, 'false_negatives': fn,
        'total_genuine': total_genuine, 'total_forgeries': total_forgeries, 'threshold': float(threshold),
        'roc_auc_bounds': [float(auc_bounds[0]), float(auc_bounds[1])], 'eer_bounds': [eer_bounds[0], eer_bounds[1]],
    }


# =============================================================================
# Model Evaluation
# =============================================================================


def evaluate_model(model: SiameseNetwork, dataloader: DataLoader, device: torch.device, threshold: float = 0.5
                   ) -> Tuple[Dict[str, float], np.ndarray, np.ndarray, np.ndarray]:
    """Evaluate a Siamese model on test data: (metrics_dict, y_true, y_scores, y_pred).  The loader may hand out fp32
    (B, 1, 64, 64) or uint8 (B, 64, 64) images (SignatureTestDataset(uint8=True))."""
    model.eval()
    all_labels: List[float] = []
    all_scores: List[float] = []
    with torch.no_grad():
        for img1, img2, labels in dataloader:
            img1 = img1.to(device)
            img2 = img2.to(device)
            _, _, similarity = model(img1, img2)
            all_labels.extend(labels.cpu().numpy().reshape(-1).tolist())
            all_scores.extend(similarity.reshape(-1).cpu().numpy().tolist())
    y_true = np.array(all_labels)
    y_scores = np.array(all_scores)
    y_pred = (y_scores >= threshold).astype(int)
    metrics = compute_verification_metrics(y_true, y_scores, y_pred, threshold)
    return metrics, y_true, y_scores, y_pred


def list_signatures(test_dir: str) -> Tuple[List[str], List[Path], np.ndarray]:
    """(writers, paths, writer_of int32 (N,)): the files SignatureTestDataset lists, writer by writer, and each file's index
    into ``writers``.  The listing alone: no sampled pairs, no np.random."""
    ds = SignatureTestDataset.__new__(SignatureTestDataset)
    ds.test_dir, ds.user_signatures = Path(test_dir), {}
    ds._load_signatures()
    writers = list(ds.user_signatures.keys())
    paths = [p for w in writers for p in ds.user_signatures[w]]
    writer_of = np.array([wi for wi, w in enumerate(writers) for _ in ds.user_signatures[w]], dtype=np.int32)
    if len(paths) < 2:
        raise ValueError(f"No test pairs in: {test_dir}")
    return writers, paths, writer_of


def evaluate_all_pairs(model: SiameseNetwork, test_dir: Union[str, Path], threshold: float = 0.5, batch_size: int = 256,
                       thresholds=None) -> Dict[str, Any]:
    """Evaluate on EVERY pair of the test directory's signatures instead of a sample: N signatures give N (N - 1) / 2 pairs,
    genuine where the writers agree.  The files are those SignatureTestDataset lists; each image is decoded once, embedded
    through the byte route, and one ``pairs`` call (same_set) yields the threshold histograms and every signature's best
    genuine and best impostor match.  ``thresholds`` replaces default_threshold_grid(threshold) (it must hold
    threshold_as_float32(threshold)).

    Returns {'metrics': metrics_from_counts' dictionary, 'num_signatures', 'num_writers', 'total_pairs', 'genuine_pairs',
    'impostor_pairs', 'rank1_identification_rate': the share of signatures that have a genuine candidate and whose best genuine
    score exceeds their best impostor score, 'hardest_impostors': per writer the highest-scoring pair with another writer}."""
    model.eval()
    writers, paths, writer_of = list_signatures(test_dir)
    device = next(model.parameters()).device
    chunks = []
    with torch.no_grad():
        for i in range(0, len(paths), batch_size):
            imgs = np.stack([load_uint8(p) for p in paths[i:i + batch_size]])
            chunks.append(model.embed_u8(torch.from_numpy(imgs).to(device)))
        emb = torch.cat(chunks, dim=0)
        ids = torch.from_numpy(writer_of).to(device)
        grid = default_threshold_grid(threshold) if thresholds is None else thresholds
        out = model.pairs(emb, ids, emb, ids, same_set=True, thresholds=grid, want_best=True)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    metrics = metrics_from_counts(host["thresholds"], host["genuine_counts"], host["impostor_counts"], threshold)
    bg, bi, bii = host["best_genuine"], host["best_impostor"], host["best_impostor_index"]
    has_genuine = host["best_genuine_index"] >= 0
    rank1 = float(np.sum(has_genuine & (bg > bi)) / len(paths))
    hardest = {}
    for wi, w in enumerate(writers):
        rows = np.where((writer_of == wi) & (bii >= 0))[0]
        if rows.size:
            r = int(rows[np.argmax(bi[rows])])                        # the first of equal maxima
            hardest[w] = {'score': float(bi[r]), 'signature': str(paths[r]), 'impostor': str(paths[int(bii[r])]),
                          'impostor_writer': writers[int(writer_of[int(bii[r])])]}
    n = len(paths)
    return {'metrics': metrics, 'num_signatures': n, 'num_writers': len(writers), 'total_pairs': n * (n - 1) // 2,
            'genuine_pairs': metrics['total_genuine'], 'impostor_pairs': metrics['total_forgeries'],
            'num_thresholds': int(host["thresholds"].size), 'rank1_identification_rate': rank1, 'hardest_impostors': hardest}


def dtw_scores(y_true: np.ndarray, distance: np.ndarray) -> Dict[str, float]:
    """{auc, eer, eer_distance} of a distance used as a verifier: -distance goes through roc_curve / auc /
    compute_eer_from_scores (labels 1 = genuine), and eer_distance is the distance at the EER point."""
    y_true, score = np.asarray(y_true), -np.asarray(distance, dtype=np.float64)
    fpr, tpr, _ = roc_curve(y_true, score)
    eer, eer_threshold = compute_eer_from_scores(y_true, score)
    return {'auc': auc(fpr, tpr), 'eer': eer, 'eer_distance': -eer_threshold}


def evaluate_dtw_baseline(test_dataset: "SignatureTestDataset", device: torch.device, band: Optional[int] = None,
                          all_pairs_dir: Optional[str] = None) -> Dict[str, Any]:
    """A training-free baseline verifier on the pairs the Siamese network is evaluated on: every pair of ``test_dataset`` (its
    resized bytes, get_uint8) is scored by the banded DTW distance between the two images' column profiles (dtw.dtw_paired,
    one HIP call), a low distance meaning genuine.  Returns {band, pairs, genuine, forgery, auc, eer, eer_distance};
    ``all_pairs_dir``: adds 'all_pairs', the same three numbers (and counts) over all N (N - 1) / 2 pairs of that directory's
    signatures, from one dtw.dtw_matrix call.  ``band`` None: dtw.default_band(64).  It needs no checkpoint; whether it tracks
    a trained verifier's accuracy is not measured."""
    from .dtw import DtwSet, check_band, dtw_matrix, dtw_paired
    band = check_band(band, IMAGE_SIZE)
    pairs = [test_dataset.get_uint8(i) for i in range(len(test_dataset))]
    first = torch.stack([p[0] for p in pairs]).to(device)
    second = torch.stack([p[1] for p in pairs]).to(device)
    y_true = np.array([int(p[2]) for p in pairs], dtype=np.int64)
    distance = dtw_paired(first, second, band).cpu().numpy()
    block: Dict[str, Any] = {'band': band, 'pairs': int(y_true.size), 'genuine': int(np.sum(y_true == 1)),
                             'forgery': int(np.sum(y_true == 0)), **dtw_scores(y_true, distance)}
    if all_pairs_dir is not None:
        _, paths, writer_of = list_signatures(all_pairs_dir)
        every = DtwSet(torch.from_numpy(np.stack([load_uint8(p) for p in paths])).to(device))
        matrix = dtw_matrix(every, band=band).cpu().numpy()
        i, j = np.triu_indices(len(paths), 1)
        same = (writer_of[i] == writer_of[j]).astype(np.int64)
        block['all_pairs'] = {'pairs': int(same.size), 'genuine': int(same.sum()), 'forgery': int(same.size - same.sum()),
                              **dtw_scores(same, matrix[i, j])}
    return block


def print_dtw_baseline_summary(block: Dict[str, Any]) -> None:
    """The --dtw_baseline line: the classical method beside the trained models."""
    line = (f"DTW BASELINE (no training, band {block['band']}): ROC-AUC {block['auc']:.4f}, EER {block['eer']:.4f} at distance "
            f"{block['eer_distance']:.0f} on {block['pairs']} pairs")
    if 'all_pairs' in block:
        ap = block['all_pairs']
        line += f"; all {ap['pairs']} pairs: ROC-AUC {ap['auc']:.4f}, EER {ap['eer']:.4f}"
    print(line)


def print_all_pairs_summary(results: Dict[str, Dict[str, Any]]) -> None:
    """The --all_pairs block: the same figures on every pair of the test directory."""
    print("ALL PAIRS")
    print("-" * 70)
    for model_name, data in results.items():
        ap = data['all_pairs']
        m = ap['metrics']
        print(f"\n{model_name.upper()}: {ap['num_signatures']} signatures of {ap['num_writers']} writers, {ap['total_pairs']} pairs "
              f"({ap['genuine_pairs']} genuine, {ap['impostor_pairs']} impostor)")
        print(f"  Accuracy:     {m['accuracy']:.4f}")
        print(f"  FAR:          {m['far']:.6f}")
        print(f"  FRR:          {m['frr']:.6f}")
        print(f"  EER:          {m['eer']:.6f}  in [{m['eer_bounds'][0]:.6f}, {m['eer_bounds'][1]:.6f}]")
        print(f"  ROC-AUC:      {m['roc_auc']:.6f}  in [{m['roc_auc_bounds'][0]:.6f}, {m['roc_auc_bounds'][1]:.6f}]")
        print(f"  Rank-1 identification rate: {ap['rank1_identification_rate']:.4f}")
    print("\n" + "=" * 70)


# =============================================================================
# Visualization (written when matplotlib can be imported)
# =============================================================================

_COLORS = ['#2ecc71', '#e74c3c', '#3498db', '#9b59b6']
_LINESTYLES = ['-', '--', '-.', ':']


def _pyplot():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except ImportError:
        return None


def _save(plt, save_path, what):
    save_path = Path(save_path)
    save_path.parent.mkdir(parents=True, exist_ok=True)
    plt.savefig(save_path, dpi=150, bbox_inches='tight')
    plt.close()
    print(f"[Plot] {what} saved to: {save_path}")


def plot_roc_curve(results: Dict[str, Dict[str, Any]], save_path: Union[str, Path], figsize: Tuple[int, int] = (10, 8)) -> bool:
    """ROC curves of all evaluated models; False (nothing written) without matplotlib."""
    plt = _pyplot()
    if plt is None:
        return False
    plt.figure(figsize=figsize)
    for idx, (model_name, data) in enumerate(results.items()):
        fpr, tpr, _ = roc_curve(data['y_true'], data['y_scores'])
        plt.plot(fpr, tpr, color=_COLORS[idx % 4], linestyle=_LINESTYLES[idx % 4], linewidth=2,
                 label=f"{model_name} (AUC = {data['metrics']['roc_auc']:.4f})")
    plt.plot([0, 1], [0, 1], 'k--', linewidth=1, label='Random Classifier')
    plt.xlim([0.0, 1.0])
    plt.ylim([0.0, 1.05])
    plt.xlabel('False Positive Rate (FAR)', fontsize=12)
    plt.ylabel('True Positive Rate (1 - FRR)', fontsize=12)
    plt.title('ROC Curve - Signature Verification', fontsize=14)
    plt.legend(loc='lower right', fontsize=10)
    plt.grid(True, alpha=0.3)
    _save(plt, save_path, "ROC curve")
    return True


def plot_det_curve(results: Dict[str, Dict[str, Any]], save_path: Union[str, Path], figsize: Tuple[int, int] = (10, 8)) -> bool:
    """DET curves (FRR vs FAR, log scale) of all evaluated models."""
    plt = _pyplot()
    if plt is None:
        return False
    plt.figure(figsize=figsize)
    for idx, (model_name, data) in enumerate(results.items()):
        fpr, fnr, _ = det_curve(data['y_true'], data['y_scores'])
        plt.plot(fpr, fnr, color=_COLORS[idx % 4], linestyle=_LINESTYLES[idx % 4], linewidth=2,
                 label=f"{model_name} (EER = {data['metrics']['eer']:.4f})")
    plt.plot([0.001, 1], [0.001, 1], 'k--', linewidth=1, label='EER Line')
    plt.xscale('log')
    plt.yscale('log')
    plt.xlim([0.001, 1])
    plt.ylim([0.001, 1])
    plt.xlabel('False Acceptance Rate (FAR)', fontsize=12)
    plt.ylabel('False Rejection Rate (FRR)', fontsize=12)
    plt.title('DET Curve - Signature Verification', fontsize=14)
    plt.legend(loc='upper right', fontsize=10)
    plt.grid(True, alpha=0.3, which='both')
    _save(plt, save_path, "DET curve")
    return True


def plot_score_distribution(results: Dict[str, Dict[str, Any]], save_path: Union[str, Path],
                            figsize: Tuple[int, int] = (12, 5)) -> bool:
    """Score histograms of genuine and forgery pairs per model."""
    plt = _pyplot()
    if plt is None:
        return False
    num_models = len(results)
    fig, axes = plt.subplots(1, num_models, figsize=(figsize[0], figsize[1]))
    if num_models == 1:
        axes = [axes]
    for idx, (model_name, data) in enumerate(results.items()):
        ax = axes[idx]
        y_true, y_scores, metrics = data['y_true'], data['y_scores'], data['metrics']
        ax.hist(y_scores[y_true == 1], bins=30, alpha=0.7, color='#2ecc71', label='Genuine', density=True,
                edgecolor='black', linewidth=0.5)
        ax.hist(y_scores[y_true == 0], bins=30, alpha=0.7, color='#e74c3c', label='Forgery', density=True,
                edgecolor='black', linewidth=0.5)
        threshold = metrics.get('eer_threshold', 0.5)
        ax.axvline(x=threshold, color='#3498db', linestyle='--', linewidth=2, label=f'EER Threshold ({threshold:.3f})')
        ax.set_xlabel('Similarity Score', fontsize=11)
        ax.set_ylabel('Density', fontsize=11)
        ax.set_title(f'{model_name}\nEER: {metrics["eer"]:.4f}', fontsize=12)
        ax.legend(loc='upper right', fontsize=9)
        ax.grid(True, alpha=0.3)
    plt.tight_layout()
    _save(plt, save_path, "Score distribution")
    return True


def plot_comparison_bar_chart(results: Dict[str, Dict[str, Any]], save_path: Union[str, Path],
                              figsize: Tuple[int, int] = (12, 6)) -> bool:
    """Bar chart of the key metrics across models."""
    plt = _pyplot()
    if plt is None:
        return False
    metrics_to_plot = ['accuracy', 'far', 'frr', 'eer', 'roc_auc', 'f1_score']
    metric_labels = ['Accuracy', 'FAR', 'FRR', 'EER', 'ROC-AUC', 'F1 Score']
    model_names = list(results.keys())
    num_models = len(model_names)
    x = np.arange(len(metrics_to_plot))
    width = 0.35 if num_models == 2 else 0.25
    fig, ax = plt.subplots(figsize=figsize)
    for idx, model_name in enumerate(model_names):
        values = [results[model_name]['metrics'][m] for m in metrics_to_plot]
        offset = (idx - (num_models - 1) / 2) * width
        bars = ax.bar(x + offset, values, width, label=model_name, color=_COLORS[idx % 4], edgecolor='black', linewidth=0.5)
        for bar, val in zip(bars, values):
            ax.annotate(f'{val:.3f}', xy=(bar.get_x() + bar.get_width() / 2, bar.get_height()), xytext=(0, 3),
                        textcoords="offset points", ha='center', va='bottom', fontsize=8)
    ax.set_xlabel('Metric', fontsize=12)
    ax.set_ylabel('Value', fontsize=12)
    ax.set_title('Model Comparison - Signature Verification Metrics', fontsize=14)
    ax.set_xticks(x)
    ax.set_xticklabels(metric_labels, fontsize=10)
    ax.legend(loc='upper right', fontsize=10)
    ax.set_ylim(0, 1.15)
    ax.grid(True, alpha=0.3, axis='y')
    plt.tight_layout()
    _save(plt, save_path, "Comparison bar chart")
    return True


# =============================================================================
# Report Generation
# =============================================================================


def generate_evaluation_report(results: Dict[str, Dict[str, Any]], output_path: Union[str, Path],
                               dtw_baseline: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """Write the evaluation report (JSON) and return it.  ``dtw_baseline``: evaluate_dtw_baseline's block, added as the
    report's 'dtw_baseline' key; no key without it."""
    report = {
        'evaluation_timestamp': datetime.now().isoformat(),
        'num_models_evaluated': len(results),
        'models': {}
    }
    for model_name, data in results.items():
        report['models'][model_name] = {
            'model_metadata': data.get('metadata', {}),
            'metrics': data['metrics'],
            'num_test_samples': len(data['y_true']),
            'genuine_samples': int(np.sum(data['y_true'] == 1)),
            'forgery_samples': int(np.sum(data['y_true'] == 0)),
        }
        if 'all_pairs' in data:
            report['models'][model_name]['all_pairs'] = data['all_pairs']

    if len(results) > 1:
        comparison = {}
        higher_is_better = ['accuracy', 'roc_auc', 'f1_score']
        for metric in ['accuracy', 'far', 'frr', 'eer', 'roc_auc', 'f1_score']:
            values = {name: data['metrics'][metric] for name, data in results.items()}
            pick = max if metric in higher_is_better else min
            comparison[metric] = {'values': values, 'best_model': pick(values.keys(), key=lambda k: values[k]),
                                  'improvement': None}
            if 'Baseline' in values and 'Augmented' in values:
                baseline_val, augmented_val = values['Baseline'], values['Augmented']
                if metric in higher_is_better:
                    improvement = ((augmented_val - baseline_val) / baseline_val * 100) if baseline_val != 0 else 0
                else:
                    improvement = ((baseline_val - augmented_val) / baseline_val * 100) if baseline_val != 0 else 0
                comparison[metric]['improvement'] = f"{improvement:+.2f}%"
        report['comparison_summary'] = comparison
    if dtw_baseline is not None:
        report['dtw_baseline'] = dtw_baseline

    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, 'w', encoding='utf-8') as f:
        json.dump(report, f, indent=2, ensure_ascii=False)
    print(f"[Report] Evaluation report saved to: {output_path}")
    return report


def print_evaluation_summary(results: Dict[str, Dict[str, Any]]) -> None:
    """Print a formatted summary of evaluation results to console."""
    print("\n" + "=" * 70)
    print("SIGNATURE VERIFICATION EVALUATION SUMMARY")
    print("=" * 70)

    for model_name, data in results.items():
        metrics = data['metrics']
        print(f"\n{model_name.upper()}")
        print("-" * 40)
        print(f"  Accuracy:     {metrics['accuracy']:.4f}")
        print(f"  FAR:          {metrics['far']:.4f}")
        print(f"  FRR:          {metrics['frr']:.4f}")
        print(f"  EER:          {metrics['eer']:.4f}")
        print(f"  ROC-AUC:      {metrics['roc_auc']:.4f}")
        print(f"  F1 Score:     {metrics['f1_score']:.4f}")
        print(f"  Precision:    {metrics['precision']:.4f}")
        print(f"  Recall:       {metrics['recall']:.4f}")
        print(f"  Specificity:  {metrics['specificity']:.4f}")
        print(f"  EER Threshold:{metrics['eer_threshold']:.4f}")
        print(f"  Confusion Matrix:")
        print(f"    TP: {metrics['true_positives']}, TN: {metrics['true_negatives']}")
        print(f"    FP: {metrics['false_positives']}, FN: {metrics['false_negatives']}")

    if len(results) > 1:
        print("\n" + "-" * 70)
        print("MODEL COMPARISON")
        print("-" * 70)
        model_names = list(results.keys())
        header = f"{'Metric':<15}"
        for name in model_names:
            header += f"{name:<15}"
        header += "Winner"
        print(header)
        print("-" * len(header))
        for metric in ['accuracy', 'far', 'frr', 'eer', 'roc_auc']:
            row = f"{metric.upper():<15}"
            values = []
            for name in model_names:
                val = results[name]['metrics'][metric]
                values.append(val)
                row += f"{val:<15.4f}"
            winner_idx = np.argmax(values) if metric in ['accuracy', 'roc_auc'] else np.argmin(values)
            row += model_names[winner_idx]
            print(row)

    print("\n" + "=" * 70)


# =============================================================================
# Main Evaluation Pipeline
# =============================================================================


def evaluate_signature_verifier(
    baseline_model_path: Optional[str],
    augmented_model_path: Optional[str],
    test_dir: str,
    output_dir: str,
    batch_size: int = 32,
    pairs_per_user: int = 20,
    threshold: float = 0.5,
    device: Optional[str] = None,
    all_pairs: bool = False,
    dtw_baseline: Optional[Union[int, str]] = None
) -> Dict[str, Any]:
    """Run the complete signature verification evaluation pipeline; returns the report dictionary.  ``all_pairs`` adds
    evaluate_all_pairs' result per model (report key 'all_pairs') and a block to the printed summary.  ``dtw_baseline``: a
    band in columns, or 'auto' for dtw.default_band(64): adds evaluate_dtw_baseline's block on the same test pairs (report key
    'dtw_baseline', with ``all_pairs`` also over every pair) and one line to the printed summary; it is not a model row."""
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"evaluate_signature_verifier: the verifier {_NO_CPU}")
    print(f"[Setup] Using device: {device}")

    output_path = Path(output_dir)
    output_path.mkdir(parents=True, exist_ok=True)

    print("\n[Setup] Loading test dataset...")
    test_dataset = SignatureTestDataset(test_dir=test_dir, pairs_per_user=pairs_per_user)
    if len(test_dataset) == 0:
        raise ValueError(f"No test pairs generated from: {test_dir}")
    test_loader = DataLoader(test_dataset, batch_size=batch_size, shuffle=False, num_workers=0)

    results: Dict[str, Dict[str, Any]] = {}
    for name, path in (('Baseline', baseline_model_path), ('Augmented', augmented_model_path)):
        if not path:
            continue
        print("\n" + "=" * 50)
        print(f"Evaluating {name.upper()} Model")
        print("=" * 50)
        model, metadata = load_model(path, device)
        metrics, y_true, y_scores, y_pred = evaluate_model(model, test_loader, device, threshold)
        results[name] = {'metrics': metrics, 'y_true': y_true, 'y_scores': y_scores, 'y_pred': y_pred, 'metadata': metadata}
        if all_pairs:
            results[name]['all_pairs'] = evaluate_all_pairs(model, test_dir, threshold)

    if not results:
        raise ValueError("At least one model path must be provided for evaluation.")

    print_evaluation_summary(results)
    if all_pairs:
        print_all_pairs_summary(results)
    baseline_block = None
    if dtw_baseline is not None:
        baseline_block = evaluate_dtw_baseline(test_dataset, device, None if dtw_baseline == 'auto' else dtw_baseline,
                                               test_dir if all_pairs else None)
        print_dtw_baseline_summary(baseline_block)

    print("\n[Plots] Generating visualizations...")
    plotted = plot_roc_curve(results, output_path / 'roc_curve.png')
    if plotted:
        plot_det_curve(results, output_path / 'det_curve.png')
        plot_score_distribution(results, output_path / 'score_distribution.png')
        if len(results) > 1:
            plot_comparison_bar_chart(results, output_path / 'comparison_metrics.png')
    else:
        print("[Plot] skipped (matplotlib not available)")

    report = generate_evaluation_report(results, output_path / 'evaluation_report.json', baseline_block)

    print("\n" + "=" * 50)
    print("EVALUATION COMPLETE")
    print("=" * 50)
    print(f"Output directory: {output_path}")
    if plotted:
        print(f"  - ROC curve: roc_curve.png")
        print(f"  - DET curve: det_curve.png")
        print(f"  - Score distribution: score_distribution.png")
        if len(results) > 1:
            print(f"  - Comparison chart: comparison_metrics.png")
    print(f"  - Report: evaluation_report.json")
    return report


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(
        description='Evaluate trained Siamese network models for signature verification',
        formatter_class=argparse.ArgumentDefaultsHelpFormatter
    )
    parser.add_argument('--baseline_model', type=str, default=None,
                        help='Path to baseline Siamese model checkpoint (.pth file)')
    parser.add_argument('--augmented_model', type=str, default=None,
                        help='Path to augmented (GAN-enhanced) Siamese model checkpoint (.pth file)')
    parser.add_argument('--test_dir', type=str, required=True,
                        help='Directory containing test signature images (organized by user)')
    parser.add_argument('--output_dir', type=str, default='./evaluation_results',
                        help='Directory to save evaluation outputs (plots, report)')
    parser.add_argument('--batch_size', type=int, default=32, help='Batch size for evaluation')
    parser.add_argument('--pairs_per_user', type=int, default=20,
                        help='Number of genuine/forgery pairs to generate per user')
    parser.add_argument('--threshold', type=float, default=0.5, help='Decision threshold for binary classification')
    parser.add_argument('--all_pairs', action='store_true',
                        help='Also evaluate on every pair of the test directory (N (N - 1) / 2 pairs) in one HIP pass')
    parser.add_argument('--device', type=str, default=None, choices=['cuda', 'cpu'],
                        help='Device to run evaluation on (default: auto-detect)')
    parser.add_argument('--dtw_baseline', nargs='?', type=lambda v: v if v == 'auto' else int(v), const='auto', default=None, metavar='BAND',
                        help='Also score the test pairs with a training-free baseline: banded dynamic time warping between the '
                             'column profiles of the two signatures, BAND columns of slack (BAND omitted: 8); adds a '
                             "'dtw_baseline' block (ROC-AUC, EER) to the report")
    args = parser.parse_args(argv)

    if not args.baseline_model and not args.augmented_model:
        parser.error("At least one of --baseline_model or --augmented_model must be provided")
    if args.device == 'cpu':
        parser.error(f"--device cpu: the verifier {_NO_CPU}")
    if args.dtw_baseline is not None and args.dtw_baseline != 'auto' and args.dtw_baseline < 0:
        parser.error("--dtw_baseline BAND must be >= 0")
    return args


def main(argv=None) -> None:
    """Main entry point with CLI argument parsing."""
    args = parse_args(argv)

    print("=" * 70)
    print("SIGNATURE VERIFICATION MODEL EVALUATION")
    print("=" * 70)
    print(f"Baseline model:  {args.baseline_model or 'Not provided'}")
    print(f"Augmented model: {args.augmented_model or 'Not provided'}")
    print(f"Test directory:  {args.test_dir}")
    print(f"Output directory:{args.output_dir}")
    print(f"Batch size:      {args.batch_size}")
    print(f"Pairs per user:  {args.pairs_per_user}")
    print(f"Threshold:       {args.threshold}")
    print("=" * 70)

    evaluate_signature_verifier(
        baseline_model_path=args.baseline_model,
        augmented_model_path=args.augmented_model,
        test_dir=args.test_dir,
        output_dir=args.output_dir,
        batch_size=args.batch_size,
        pairs_per_user=args.pairs_per_user,
        threshold=args.threshold,
        device=args.device,
        all_pairs=args.all_pairs,
        dtw_baseline=args.dtw_baseline
    )


if __name__ == '__main__':
    main()
