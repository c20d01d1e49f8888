"""Drop-in for the reference's ``utils/metrics.py`` on the MI355X HIP engine.

The stroke statistics (utils/metrics.py:118-174) are per-image pixel counts below a threshold.  Here the counting is done
on the device -- by the Generator's last kernel for generated batches (Engine.g_generate_u8) or by ``siggan_image_stats``
for any other tensor -- and only three int32 per image reach the host; the dictionaries are then formed from the counts
with the numpy calls the reference makes on its per-image densities.  A per-image density is count / P in fp32: exact for
the image sizes built here (P a power of two, count < 2**24), so it equals the reference's mean over 0/1 floats bit for bit;
for another P the two may differ in the last bit.

FID and LPIPS need downloaded network weights; computing them is not built.  The availability flags and the ImportError
texts are the reference's, so callers (the evaluation CLI) report them the same way.  What IS built is the same
construction over a network the user trains here: ``calculate_verifier_frechet_distance``, a Frechet distance between two
image sets in the Siamese verifier's embedding space (utils/frechet.py; the statistics are accumulated on the device),
and ``calculate_verifier_manifold_metrics``: precision / recall, density / coverage and nearest-real distances in that space
(utils/neighbors.py; exact fp64 nearest-neighbour queries on the device), and ``calculate_verifier_two_sample``: the Kernel
Inception Distance and a permutation test of the kernel MMD in that space (utils/twosample.py; fp64 quadratic forms of the
implicit kernel matrix on the device)."""
from collections import defaultdict
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from .._lib import IS_INK_SIGNED, IS_INK_UNIT, IS_NEG
from .frechet import FeatureMoments, embedding_spread, frechet_distance
from .neighbors import manifold_metrics
from .twosample import kid, mmd_permutation_test

try:
    from torchvision.models import inception_v3  # noqa: F401
    INCEPTION_AVAILABLE = True
except ImportError:
    INCEPTION_AVAILABLE = False

try:
    import lpips  # noqa: F401
    LPIPS_AVAILABLE = True
except ImportError:
    LPIPS_AVAILABLE = False


def calculate_fid(real_images: torch.Tensor, fake_images: torch.Tensor, device: Optional[torch.device] = None) -> float:
    if not INCEPTION_AVAILABLE:
        raise ImportError("torchvision required for FID calculation")
    raise NotImplementedError("FID needs InceptionV3 weights, which this build does not ship or download")


def calculate_lpips_diversity(images_list: List[torch.Tensor], device: Optional[torch.device] = None) -> float:
    if not LPIPS_AVAILABLE:
        raise ImportError("lpips package required: pip install lpips")
    raise NotImplementedError("LPIPS needs AlexNet weights, which this build does not ship or download")


# ---- Frechet distance over verifier embeddings (device moments, host root) ---------------------------------------------
def verifier_embedding_chunks(images: torch.Tensor, verifier, max_batch: Optional[int] = None):
    """Embed ``images`` -- fp32 (N, 1, 64, 64) in [-1, 1] or uint8 (N, 64, 64), on the verifier's device -- in chunks of at
    most min(max_batch, verifier.max_images); yields every chunk's (b, E) fp32 embeddings, which stay on the device."""
    if images.dtype == torch.uint8:
        embed = verifier.embed_u8
    elif images.dtype == torch.float32:
        embed = getattr(verifier, "forward_one", verifier)          # SiameseNetwork.forward_one / CNNEncoder.forward
    else:
        raise ValueError(f"images must be float32 or uint8, got {images.dtype}")
    step = int(verifier.max_images) if max_batch is None else max(1, min(int(max_batch), int(verifier.max_images)))
    for i in range(0, images.shape[0], step):
        yield embed(images[i:i + step])


def accumulate_verifier_moments(moments: FeatureMoments, images: torch.Tensor, verifier, max_batch: Optional[int] = None) -> None:
    """Add the embeddings of ``images`` (``verifier_embedding_chunks``) to ``moments``; nothing reaches the host."""
    for emb in verifier_embedding_chunks(images, verifier, max_batch):
        moments.update(emb)


def calculate_verifier_frechet_distance(real_images: torch.Tensor, fake_images: torch.Tensor, verifier,
                                        max_batch: Optional[int] = None) -> Dict[str, Any]:
    """Frechet distance between two image sets in the embedding space of ``verifier`` (a signature_verifier_eval
    SiameseNetwork or CNNEncoder in eval mode on a ROCm device).  Each set: fp32 (N, 1, 64, 64) in [-1, 1] or uint8
    (N, 64, 64), N >= 2.  -> {'frechet_distance', 'spread_real', 'spread_generated', 'n_real', 'n_generated',
    'embedding_dim'}; a spread is tr(cov) of the set's embeddings (utils.frechet.embedding_spread)."""
    dev = next(verifier.parameters()).device
    dim = int(verifier.embedding_dim)
    stats = []
    for images in (real_images, fake_images):
        if images.shape[0] < 2:
            raise ValueError(f"a covariance needs at least 2 images per set, got {images.shape[0]}")
        moments = FeatureMoments(dim, dev)
        try:
            accumulate_verifier_moments(moments, images.to(dev), verifier, max_batch)
            stats.append(moments.finish())
        finally:
            moments.close()
    (n_r, mu_r, cov_r), (n_f, mu_f, cov_f) = stats
    return {"frechet_distance": frechet_distance(mu_r, cov_r, mu_f, cov_f), "spread_real": embedding_spread(cov_r),
            "spread_generated": embedding_spread(cov_f), "n_real": n_r, "n_generated": n_f, "embedding_dim": dim}


# ---- precision / recall / nearest-real distances over verifier embeddings (device k-NN, host means) ------------------
def verifier_embeddings(images: torch.Tensor, verifier, max_batch: Optional[int] = None) -> torch.Tensor:
    """The (N, E) fp32 embeddings of ``images`` in one device buffer, embedded by the chunked route of the moments."""
    with torch.no_grad():
        chunks = [emb.detach().to(torch.float32) for emb in verifier_embedding_chunks(images, verifier, max_batch)]
    if not chunks:
        return torch.empty(0, int(verifier.embedding_dim), dtype=torch.float32, device=images.device)
    return torch.cat(chunks, dim=0).contiguous()


def calculate_verifier_manifold_metrics(real_images: torch.Tensor, fake_images: torch.Tensor, verifier, k: int = 3,
                                        max_batch: Optional[int] = None) -> Dict[str, Any]:
    """Improved precision / recall, density / coverage and nearest-real distances of two image sets in the embedding
    space of ``verifier`` (as for ``calculate_verifier_frechet_distance``: the same image formats, the same chunks).  More
    than k images per set, else ValueError.  -> utils.neighbors.manifold_metrics' dictionary plus 'embedding_dim'."""
    dev = next(verifier.parameters()).device
    if real_images.shape[0] <= k or fake_images.shape[0] <= k:
        raise ValueError(f"the k-th neighbour inside a set needs more than k = {k} images per set, got "
                         f"{real_images.shape[0]} and {fake_images.shape[0]}")
    real_emb = verifier_embeddings(real_images.to(dev), verifier, max_batch)
    fake_emb = verifier_embeddings(fake_images.to(dev), verifier, max_batch)
    out = manifold_metrics(real_emb, fake_emb, k)
    out["embedding_dim"] = int(verifier.embedding_dim)
    return out


# ---- KID and the MMD permutation test over verifier embeddings (device quadratic forms, host statistics) ---------------
def two_sample_metrics(real_emb: torch.Tensor, fake_emb: torch.Tensor, permutations: int = 1000, subsets: int = 100,
                       seed: int = 0) -> Dict[str, Any]:
    """{'kid': utils.twosample.kid's dictionary, 'mmd_test': utils.twosample.mmd_permutation_test's (RBF, median
    heuristic), 'n_real', 'n_generated'} of two (n, dim) fp32 embedding sets on one ROCm device."""
    return {"kid": kid(real_emb, fake_emb, subsets=subsets, seed=seed),
            "mmd_test": mmd_permutation_test(real_emb, fake_emb, permutations=permutations, seed=seed),
            "n_real": int(real_emb.shape[0]), "n_generated": int(fake_emb.shape[0])}


def calculate_verifier_two_sample(real_images: torch.Tensor, fake_images: torch.Tensor, verifier, permutations: int = 1000,
                                  subsets: int = 100, seed: int = 0, max_batch: Optional[int] = None) -> Dict[str, Any]:
    """The Kernel Inception Distance and the RBF MMD permutation test of two image sets in the embedding space of ``verifier``
    (as for ``calculate_verifier_frechet_distance``: the same image formats, the same chunks).  At least 2 images per set,
    else ValueError.  -> ``two_sample_metrics``' dictionary plus 'embedding_dim'."""
    dev = next(verifier.parameters()).device
    if real_images.shape[0] < 2 or fake_images.shape[0] < 2:
        raise ValueError(f"a two-sample statistic needs at least 2 images per set, got {real_images.shape[0]} and "
                         f"{fake_images.shape[0]}")
    real_emb = verifier_embeddings(real_images.to(dev), verifier, max_batch)
    fake_emb = verifier_embeddings(fake_images.to(dev), verifier, max_batch)
    out = two_sample_metrics(real_emb, fake_emb, permutations, subsets, seed)
    out["embedding_dim"] = int(verifier.embedding_dim)
    return out


# ---- counters -> dictionaries (pure numpy) ---------------------------------------------------------------------------
def densities_from_counts(counts, pixels: int, signed: Optional[bool] = None) -> np.ndarray:
    """Per-image fraction of pixels below the threshold, float32 (N,), from (N, 3) counters (columns _lib.IS_*).
    ``signed`` None: the reference's test ``images.min() < 0`` over the whole batch, i.e. any NEG count non-zero; True /
    False pick the [-1, 1] / [0, 1] branch outright."""
    counts = np.asarray(counts).reshape(-1, 3)
    if signed is None:
        signed = bool(counts[:, IS_NEG].sum() > 0)
    ink = counts[:, IS_INK_SIGNED if signed else IS_INK_UNIT]
    return ink.astype(np.float32) / np.float32(pixels)


def _stroke_dict(d: np.ndarray) -> Dict[str, float]:
    return {"mean": float(np.mean(d)), "std": float(np.std(d)), "min": float(np.min(d)), "max": float(np.max(d))}


def _foreground_dict(d: np.ndarray) -> Dict[str, object]:
    return {"mean": float(np.mean(d)), "std": float(np.std(d)),
            "percentiles": {q: float(np.percentile(d, int(q))) for q in ("25", "50", "75")}}


def stroke_density_from_counts(counts, pixels: int, signed: Optional[bool] = None) -> Dict[str, float]:
    """calculate_stroke_density's dictionary from ready counters (what the evaluation CLI holds after generation)."""
    return _stroke_dict(densities_from_counts(counts, pixels, signed))


def foreground_ratio_from_counts(counts, pixels: int, signed: Optional[bool] = None) -> Dict[str, object]:
    """calculate_foreground_ratio's dictionary from ready counters."""
    return _foreground_dict(densities_from_counts(counts, pixels, signed))


# ---- tensors -> counters (device) ------------------------------------------------------------------------------------
def _densities(images: torch.Tensor, threshold: float) -> np.ndarray:
    from ..engine import Engine
    if images.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("the stroke statistics are counted on a ROCm device ('cuda:N'); there is no CPU path")
        images = images.cuda()
    x = images.detach().to(torch.float32)
    signed = None
    if x.dim() == 4 and x.shape[1] > 1:
        # more than one channel: the reference maps to [0, 1] first (when any value is negative) and averages the
        # channels (utils/metrics.py:129-133); torch does both, the kernel counts the one-channel result's unit branch
        if bool(x.min() < 0):
            x = (x + 1) / 2
        x = x.mean(dim=1, keepdim=True)
        signed = False
    x = x.contiguous()
    counts = Engine.image_stats(x, threshold).cpu().numpy()
    return densities_from_counts(counts, x.numel() // x.shape[0], signed)


def calculate_stroke_density(images: torch.Tensor, threshold: float = 0.5) -> Dict[str, float]:
    """images (N, C, H, W) in [0, 1] or [-1, 1] -> {'mean', 'std', 'min', 'max'} of the per-image stroke density."""
    return _stroke_dict(_densities(images, threshold))


def calculate_foreground_ratio(images: torch.Tensor, threshold: float = 0.5) -> Dict[str, object]:
    """images (N, C, H, W) in [0, 1] or [-1, 1] -> {'mean', 'std', 'percentiles': {'25', '50', '75'}}."""
    return _foreground_dict(_densities(images, threshold))


# ---- fragmentation: connected ink components (components.py) ------------------------------------------------------------
def fragmentation_from_counters(counters) -> Dict[str, Any]:
    """The fragmentation dictionary from (N, 9) component counters (components.STAT_NAMES), pure numpy on integers:
    components_mean / components_median: ink components per image; small_components_mean: those below min_area;
    speckle_ink_ratio: sum of small_ink over sum of ink (0.0 without any ink); largest_component_share_mean: the mean of
    largest / ink over the images that have ink (None when none has); empty_images: images without ink; n."""
    from ..components import COMPONENTS, INK, LARGEST, SMALL_COMPONENTS, SMALL_INK
    c = np.asarray(counters, dtype=np.int64).reshape(-1, 9)
    if c.shape[0] == 0:
        raise ValueError("no images")
    if (c[:, COMPONENTS] < 0).any():
        raise RuntimeError("siggan_components_u8 hit its safety bound (COMPONENTS = -1): a bug in the kernel, not an input")
    ink = c[:, INK]
    has = ink > 0
    total = int(ink.sum())
    return {"components_mean": float(np.mean(c[:, COMPONENTS])), "components_median": float(np.median(c[:, COMPONENTS])),
            "small_components_mean": float(np.mean(c[:, SMALL_COMPONENTS])),
            "speckle_ink_ratio": float(int(c[:, SMALL_INK].sum()) / total) if total else 0.0,
            "largest_component_share_mean": float(np.mean(c[has, LARGEST] / ink[has])) if has.any() else None,
            "empty_images": int((~has).sum()), "n": int(c.shape[0])}


def quantize_generated(images: torch.Tensor) -> torch.Tensor:
    """fp32 in [-1, 1] -> uint8 by the generation rule ((x + 1) * 127.5, clip to 0..255, truncate), where the tensor lives."""
    return ((images.detach().to(torch.float32) + 1) * 127.5).clamp(0, 255).to(torch.uint8)


def calculate_fragmentation(images: torch.Tensor, threshold: int = 128, connectivity: int = 8,
                            min_area: Optional[int] = None) -> Dict[str, Any]:
    """How broken up the ink of ``images`` is: uint8 (B, S, S) / (B, 1, S, S), or fp32 in [-1, 1] quantised by the generation
    rule first.  Ink is byte < ``threshold``; ``min_area`` None: components.default_min_area.  The components are labelled on
    the device (components.component_stats) and only the (B, 9) counters reach the host; a structural metric that needs
    no network weights.  Returns fragmentation_from_counters' dictionary."""
    from ..components import component_stats
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"images must be a tensor, got {type(images).__name__}")
    if images.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("the components are labelled on a ROCm device ('cuda:N'); there is no CPU path")
        images = images.cuda()
    if images.dtype != torch.uint8:
        images = quantize_generated(images)
    return fragmentation_from_counters(component_stats(images.contiguous(), threshold, connectivity, min_area).cpu().numpy())


# ---- stroke geometry: skeleton and pen width (strokes.py) ---------------------------------------------------------------
def _ceil_sqrt(values: np.ndarray) -> np.ndarray:
    """The smallest integer k with k * k >= v, by integer comparison (v in 0..4096)."""
    squares = np.arange(0, 66, dtype=np.int64) ** 2
    return np.searchsorted(squares, np.asarray(values, dtype=np.int64), side="left")


def stroke_geometry_from_counters(counters) -> Dict[str, Any]:
    """The stroke-geometry dictionary from (N, 23) stroke counters (strokes.STAT_NAMES), pure numpy on integers.
    images: N; bound_hit: images whose thinning reached the kernel's safety bound (PASSES = -1; they count in nothing below);
    empty: images without ink; width_histogram: the sixteen width bins summed over the images; mean_width:
    sum((2k - 1) * hist[k]) / sum(hist), the pooled local pen width (None without a skeleton); width_per_image {mean, std}: the
    same per image, over the images that have a skeleton; thickest {mean, max}: 2 * ceil(sqrt(d2_max)) - 1 per image, over the
    images that have ink; skeleton_length {mean, std}; endpoints {mean}; junction_pixels {mean}; ink_per_skeleton_pixel {mean}:
    ink / skeleton per image, over the images that have a skeleton.  A bar of even width reads one pixel low (strokes.py)."""
    from ..strokes import COUNT, D2_MAX, ENDPOINTS, INK, JUNCTION_PIXELS, PASSES, SKELETON, WIDTH_BINS, WIDTH_HIST
    c = np.asarray(counters, dtype=np.int64).reshape(-1, COUNT)
    if c.shape[0] == 0:
        raise ValueError("no images")
    n = int(c.shape[0])
    hit = c[:, PASSES] < 0
    c = c[~hit]
    hist = c[:, WIDTH_HIST:WIDTH_HIST + WIDTH_BINS]
    widths = 2 * np.arange(1, WIDTH_BINS + 1, dtype=np.int64) - 1
    pooled = hist.sum(axis=0)
    has_skel, has_ink = c[:, SKELETON] > 0, c[:, INK] > 0
    per_image = (hist[has_skel] * widths).sum(axis=1) / np.maximum(hist[has_skel].sum(axis=1), 1)
    thickest = 2 * _ceil_sqrt(c[has_ink, D2_MAX]) - 1
    mean = lambda v: float(np.mean(v)) if len(v) else None                        # noqa: E731
    std = lambda v: float(np.std(v)) if len(v) else None                          # noqa: E731
    return {"images": n, "empty": int((~has_ink).sum()), "bound_hit": int(hit.sum()),
            "width_histogram": [int(v) for v in pooled],
            "mean_width": float(int((pooled * widths).sum()) / int(pooled.sum())) if pooled.sum() else None,
            "width_per_image": {"mean": mean(per_image), "std": std(per_image)},
            "thickest": {"mean": mean(thickest), "max": int(thickest.max()) if len(thickest) else None},
            "skeleton_length": {"mean": mean(c[:, SKELETON]), "std": std(c[:, SKELETON])},
            "endpoints": {"mean": mean(c[:, ENDPOINTS])}, "junction_pixels": {"mean": mean(c[:, JUNCTION_PIXELS])},
            "ink_per_skeleton_pixel": {"mean": mean(c[has_skel, INK] / np.maximum(c[has_skel, SKELETON], 1))}}


def calculate_stroke_geometry(images: torch.Tensor, threshold: int = 128) -> Dict[str, Any]:
    """How thick and how long the strokes of ``images`` are: uint8 (B, S, S) / (B, 1, S, S), or fp32 in [-1, 1] quantised by the
    generation rule first.  Ink is byte < ``threshold``.  Skeleton and distance map are computed on the device
    (strokes.stroke_stats) and only the (B, 23) counters reach the host; a structural metric that needs no network weights.
    Returns stroke_geometry_from_counters' dictionary."""
    from ..strokes import stroke_stats
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"images must be a tensor, got {type(images).__name__}")
    if images.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("the strokes are measured on a ROCm device ('cuda:N'); there is no CPU path")
        images = images.cuda()
    if images.dtype != torch.uint8:
        images = quantize_generated(images)
    return stroke_geometry_from_counters(stroke_stats(images.contiguous(), threshold).cpu().numpy())


# ---- shape attributes: ink moments (shape.py) --------------------------------------------------------------------------------
def shape_attributes_from_features(features) -> Dict[str, Any]:
    """The shape-attribute dictionary from (N, 8) features (shape.FEATURES), pure numpy: {images, empty, and per feature name
    {mean, std, p5, p50, p95}}.  mass is summarised over every image, the other seven over the images that have ink (None where
    there is none): an empty image has no centre, size or slant.  A signature leaning to the right has a NEGATIVE slant."""
    from ..shape import FEATURES, MASS
    f = np.asarray(features, dtype=np.float64).reshape(-1, len(FEATURES))
    if f.shape[0] == 0:
        raise ValueError("no images")
    has = f[:, MASS] > 0.0
    out: Dict[str, Any] = {"images": int(f.shape[0]), "empty": int((~has).sum())}
    for k, name in enumerate(FEATURES):
        v = f[:, k] if k == MASS else f[has, k]
        if len(v) == 0:
            out[name] = None
            continue
        p5, p50, p95 = np.percentile(v, [5, 50, 95])
        out[name] = {"mean": float(np.mean(v)), "std": float(np.std(v)), "p5": float(p5), "p50": float(p50), "p95": float(p95)}
    return out


def calculate_shape_attributes(images: torch.Tensor) -> Dict[str, Any]:
    """Where the ink of ``images`` sits, how far it spreads and how it leans: uint8 (B, S, S) / (B, 1, S, S) -- exact integer sums
    on the device (shape.shape_sums_u8), turned into features on the host (shape.features_from_sums) -- or fp32 in [-1, 1]
    (shape.shape_features, fp64 on the device), S = 64 or 128.  Only (B, 6) or (B, 8) numbers reach the host; a structural
    metric that needs no network weights.  Returns shape_attributes_from_features' dictionary."""
    from ..shape import features_from_sums, shape_features, shape_sums_u8
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"images must be a tensor, got {type(images).__name__}")
    if images.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("the moments are summed on a ROCm device ('cuda:N'); there is no CPU path")
        images = images.cuda()
    if images.dtype == torch.uint8:
        return shape_attributes_from_features(features_from_sums(shape_sums_u8(images.contiguous()).cpu().numpy(), images.shape[-1]))
    return shape_attributes_from_features(shape_features(images.detach().to(torch.float32).contiguous()).cpu().numpy())


# ---- pixel-space similarity: SSIM (ssim.py) ---------------------------------------------------------------------------------
SSIM_DIVERSITY_IMAGES = 512           # a set's diversity is taken over at most its first 512 images (131 k pairs)


def _image_set(images, what: str, set_class, op: str):
    """A ``set_class`` (ssim.SsimSet, dtw.DtwSet) of ``images``: one as it is; uint8 (N, H, W) / (N, 1, H, W) or fp32 in [-1, 1], quantised
    by the generation rule first, moved to the device when it is not there.  ``op``: the measure, as the refusal names it."""
    if isinstance(images, set_class):
        return images
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"{what} must be a tensor, got {type(images).__name__}")
    if images.device.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError(f"{op} is computed on a ROCm device ('cuda:N'); there is no CPU path")
        images = images.cuda()
    if images.dtype != torch.uint8:
        images = quantize_generated(images)
    return set_class(images.contiguous())


def calculate_ssim_diversity(images, max_images: int = SSIM_DIVERSITY_IMAGES) -> Dict[str, Any]:
    """Mean pairwise SSIM of a set and 1 - mean (higher = more diverse, the direction of LPIPS), over at most its first
    ``max_images`` images: ssim.ssim_diversity of the set's own matrix, which is formed on the device.  A pixel-space measure
    that needs no network weights."""
    from ..ssim import SsimSet, ssim_diversity, ssim_matrix
    s = _image_set(images, "images", SsimSet, "SSIM")
    if s.n > max_images:
        s = SsimSet(s.u8[:max_images])
    return ssim_diversity(ssim_matrix(s).cpu().numpy())


def calculate_ssim_nearest_real(generated, real) -> Dict[str, Any]:
    """Each generated image's highest SSIM to a real one against the real set's own leave-one-out values
    (ssim.nearest_real_from_best): the memorisation check in pixel space.  Only one value and one index per image leave the
    device; no matrix is formed."""
    from ..ssim import SsimSet, nearest_real_from_best, ssim_best
    g, r = _image_set(generated, "generated", SsimSet, "SSIM"), _image_set(real, "real", SsimSet, "SSIM")
    best, index = ssim_best(g, r)
    loo = ssim_best(r)[0].cpu().numpy() if r.n >= 2 else None
    return nearest_real_from_best(best.cpu().numpy(), index.cpu().numpy(), loo)


# ---- elastic similarity: banded DTW on column profiles (dtw.py) ---------------------------------------------------------------
DTW_DIVERSITY_IMAGES = 512            # as for SSIM: a set's diversity is taken over at most its first 512 images


def calculate_dtw_diversity(images, band: Optional[int] = None, max_images: int = DTW_DIVERSITY_IMAGES) -> Dict[str, Any]:
    """Mean pairwise DTW distance of a set per column (higher = more diverse, the direction of LPIPS), over at most its first
    ``max_images`` images: dtw.dtw_diversity of the set's own matrix, which is formed on the device.  The same signature
    nudged sideways counts as the same, genuinely different shapes as different; it needs no network weights."""
    from ..dtw import DtwSet, dtw_diversity, dtw_matrix
    s = _image_set(images, "images", DtwSet, "DTW")
    if s.n > max_images:
        s = s.first(max_images)
    return dtw_diversity(dtw_matrix(s, band=band).cpu().numpy(), s.w)


def calculate_dtw_nearest_real(generated, real, band: Optional[int] = None) -> Dict[str, Any]:
    """Each generated image's lowest DTW distance to a real one against the real set's own leave-one-out values
    (dtw.nearest_real_from_best): the memorisation check of --ssim made tolerant of small shifts.  Only one value and one
    index per image leave the device; no matrix is formed."""
    from ..dtw import DtwSet, dtw_best, nearest_real_from_best
    g, r = _image_set(generated, "generated", DtwSet, "DTW"), _image_set(real, "real", DtwSet, "DTW")
    best, index = dtw_best(g, r, band)
    loo = dtw_best(r, band=band)[0].cpu().numpy() if r.n >= 2 else None
    return nearest_real_from_best(best.cpu().numpy(), index.cpu().numpy(), loo, g.w)


# ---- mode coverage: k-means bins, NDB and JS divergence (utils/modes.py) -------------------------------------------------------
def mode_features(images: torch.Tensor, verifier=None, max_batch: Optional[int] = None) -> torch.Tensor:
    """The fp32 rows mode counting works on.  With a ``verifier``: its embeddings (``verifier_embeddings``: the same image
    formats and chunks as the other verifier metrics).  Without one: modes.pixel_features of the bytes -- uint8 (N, S, S) /
    (N, 1, S, S) as they are, fp32 in [-1, 1] quantised by the generation rule first --, which needs no network weights."""
    from .modes import pixel_features
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"images must be a tensor, got {type(images).__name__}")
    dev = next(verifier.parameters()).device if verifier is not None else images.device
    if dev.type != "cuda":
        if not torch.cuda.is_available():
            raise RuntimeError("the modes are counted on a ROCm device ('cuda:N'); there is no CPU path")
        dev = torch.device("cuda")
    images = images.to(dev)
    if verifier is not None:
        return verifier_embeddings(images, verifier, max_batch)
    return pixel_features(images if images.dtype == torch.uint8 else quantize_generated(images))


def calculate_mode_coverage(real_images: torch.Tensor, fake_images: torch.Tensor, verifier=None, **kw) -> Dict[str, Any]:
    """Which groups of the real set the generated set produces too rarely or not at all: the number of statistically
    different bins and the JS divergence of the bin histograms over k-means bins of the real set, beside the real set's own
    hold-out floor (modes.mode_coverage; ``kw``: its k, seed, alpha, iterations, restarts).  Features: ``mode_features``.
    -> mode_coverage's dictionary plus 'feature_space' ('verifier' or 'pixels/4') and 'feature_dim'."""
    from .modes import mode_coverage
    real, fake = mode_features(real_images, verifier), mode_features(fake_images, verifier)
    out = mode_coverage(real, fake, **kw)
    out["feature_space"], out["feature_dim"] = ("verifier" if verifier is not None else "pixels/4"), int(real.shape[1])
    return out


class MetricsTracker:
    """Per-epoch running values and the history of their epoch averages (utils/metrics.py:177-213)."""

    def __init__(self) -> None:
        self.metrics: Dict[str, List[float]] = defaultdict(list)
        self.epoch_metrics: Dict[str, List[float]] = defaultdict(list)

    def add(self, name: str, value: Union[float, torch.Tensor]) -> None:
        self.epoch_metrics[name].append(value.item() if isinstance(value, torch.Tensor) else value)

    def get_average(self, name: str) -> float:
        values = self.epoch_metrics.get(name, [])
        return float(np.mean(values)) if values else 0.0

    def get_all_averages(self) -> Dict[str, float]:
        return {name: self.get_average(name) for name in self.epoch_metrics}

    def reset(self) -> None:
        """Close the epoch: every metric's average joins its history, the running values are dropped."""
        for name, values in self.epoch_metrics.items():
            if values:
                self.metrics[name].append(float(np.mean(values)))
        self.epoch_metrics.clear()

    def get_history(self, name: str) -> List[float]:
        return self.metrics.get(name, [])

    def get_last(self, name: str, default: float = 0.0) -> float:
        history = self.metrics.get(name, [])
        return history[-1] if history else default
