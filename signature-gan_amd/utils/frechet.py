"""Frechet distance between two sets of feature vectors whose statistics were accumulated on the device.

The reference's ``calculate_fid`` (utils/metrics.py:68-78) copies every feature vector to the host and forms ``np.cov``
there.  Here the features never leave the device: ``FeatureMoments`` (include/siggan_moments.h, csrc/moments.hip) adds
every batch's sum vector and Gram matrix to an fp64 accumulator, and only dim * (dim + 1) doubles come back at the end.
Mean and covariance follow from them on the host, and so does the distance: a matrix square root of a D <= 1024 matrix
belongs there.  The features this package uses are the Siamese verifier's embeddings (``utils.metrics.
calculate_verifier_frechet_distance``): the FID construction with weights the user trains here instead of InceptionV3's."""
import ctypes as C
from typing import Tuple

import numpy as np
import torch

from .. import _lib
from .._call import check_rows, ptr, stream


def stats_from_moments(n: int, s: np.ndarray, gram: np.ndarray) -> Tuple[int, np.ndarray, np.ndarray]:
    """(n, mean, cov) from the row count, the sum vector s (D) and the Gram matrix G (D, D) of n rows:
    mean = s / n, cov = (G - n mean mean^T) / (n - 1) as ``np.cov(x, rowvar=False)`` defines it, symmetrised; fp64."""
    n = int(n)
    if n < 2:
        raise ValueError(f"a covariance needs at least 2 feature rows, got {n}")
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    gram = np.asarray(gram, dtype=np.float64).reshape(s.size, s.size)
    mean = s / n
    cov = (gram - np.outer(s, s) / n) / (n - 1)           # n mean mean^T = s s^T / n: one rounding fewer
    return n, mean, (cov + cov.T) / 2


class FeatureMoments:
    """Streaming fp64 moments of (n, dim) fp32 feature batches on a ROCm device; no call synchronises the host before
    ``finish`` copies the result back."""

    def __init__(self, dim: int, device) -> None:
        self.lib = _lib.load()
        self.dim = int(dim)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("FeatureMoments accumulates on a ROCm device ('cuda:N'); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        h = C.c_void_p()
        _lib.check(self.lib.siggan_moments_create(device.index, self.dim, C.byref(h)))
        self._h = h

    def _stream(self):
        return stream(self.device)

    def update(self, features: torch.Tensor) -> None:
        """features: (n, dim) fp32 contiguous tensor on this accumulator's device, n >= 1."""
        check_rows("features", features, torch.float32, f"(n, {self.dim})", shape=(None, self.dim), device=self.device,
                   where=str(self.device))
        _lib.check(self.lib.siggan_moments_update(self._h, ptr(features), features.shape[0], self._stream()))

    def reset(self) -> None:
        _lib.check(self.lib.siggan_moments_reset(self._h, self._stream()))

    @property
    def count(self) -> int:
        n = C.c_int64()
        _lib.check(self.lib.siggan_moments_read(self._h, None, None, C.byref(n), self._stream()))
        return int(n.value)

    def read(self) -> Tuple[int, np.ndarray, np.ndarray]:
        """(count, s (dim), G (dim, dim)) as numpy fp64: the raw accumulator."""
        s = torch.empty(self.dim, dtype=torch.float64, device=self.device)
        g = torch.empty(self.dim, self.dim, dtype=torch.float64, device=self.device)
        n = C.c_int64()
        _lib.check(self.lib.siggan_moments_read(self._h, ptr(s), ptr(g), C.byref(n), self._stream()))
        return int(n.value), s.cpu().numpy(), g.cpu().numpy()

    def finish(self) -> Tuple[int, np.ndarray, np.ndarray]:
        """(n, mean (dim), cov (dim, dim)) of every row since the last reset; ValueError for n < 2."""
        n = self.count
        if n < 2:
            raise ValueError(f"a covariance needs at least 2 feature rows, got {n}")
        return stats_from_moments(*self.read())

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.siggan_moments_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # interpreter shutdown
            pass


def frechet_distance(mu1: np.ndarray, sigma1: np.ndarray, mu2: np.ndarray, sigma2: np.ndarray) -> float:
    """||mu1 - mu2||^2 + tr(sigma1 + sigma2 - 2 (sigma1 sigma2)^(1/2)) in fp64 on the host.  The root is
    ``scipy.linalg.sqrtm``; a complex round-off part of it is dropped (what the reference's calculate_fid ends with)."""
    from scipy import linalg
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape or sigma1.shape != (mu1.size, mu1.size) or sigma2.shape != sigma1.shape:
        raise ValueError(f"shapes do not agree: mu {mu1.shape} / {mu2.shape}, sigma {sigma1.shape} / {sigma2.shape}")
    root = linalg.sqrtm(sigma1 @ sigma2)
    if np.iscomplexobj(root):
        root = root.real
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(sigma1 + sigma2 - 2 * root))


def embedding_spread(cov: np.ndarray) -> float:
    """tr(cov): for unit-norm embeddings n / (n - 1) * (1 - ||mean||^2), i.e. half the mean squared distance between two
    different samples -- a diversity figure the moments give for free."""
    return float(np.trace(np.asarray(cov, dtype=np.float64)))
