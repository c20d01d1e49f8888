"""Shared by the uint8-generation / stroke-statistics tests: the per-image counters in numpy float32 arithmetic and the
reference's two statistics (utils/metrics.py:118-174) restated with torch on the CPU."""
import numpy as np
import torch


def numpy_counts(x, thr):
    """[NEG, INK_SIGNED, INK_UNIT] per image of fp32 images x (B, ...), every operation in float32 (include/siggan.h)."""
    x = np.asarray(x, np.float32)
    x = x.reshape(x.shape[0], -1)
    one, half, t = np.float32(1.0), np.float32(0.5), np.float32(thr)
    return np.stack([(x < np.float32(0.0)).sum(1), ((x + one) * half < t).sum(1), (x < t).sum(1)], axis=1).astype(np.int64)


def torch_densities(images, thr=0.5):
    """Per-image fraction of pixels under the threshold as the reference forms it: map to [0, 1] when any value is negative,
    average the channels, compare, mean of the 0/1 floats per image.  images: (N, C, H, W) CPU tensor."""
    images = images.detach().float().cpu()
    if images.min() < 0:
        images = (images + 1) / 2
    if images.shape[1] > 1:
        images = images.mean(dim=1, keepdim=True)
    return (images < thr).float().view(images.shape[0], -1).mean(dim=1).numpy()


def stroke_dict(d):
    return {"mean": float(np.mean(d)), "std": float(np.std(d)), "min": float(np.min(d)), "max": float(np.max(d))}


def foreground_dict(d):
    return {"mean": float(np.mean(d)), "std": float(np.std(d)),
            "percentiles": {"25": float(np.percentile(d, 25)), "50": float(np.percentile(d, 50)), "75": float(np.percentile(d, 75))}}
