"""Drop-in for the reference's ``evaluate_vanilla_gan_signatures.py`` CLI on the MI355X HIP engine: checkpoint in ->
generated samples -> sample grids, stroke / foreground statistics (against a folder of real images when one is given)
and a JSON report.  Flags, function names, stdout lines, report keys and exit codes follow
evaluate_vanilla_gan_signatures.py:44-612.

What differs is where the work happens.  Generation goes through ``Engine.g_generate_u8`` with the stroke counters: the
Generator's last kernel counts the pixels itself, so evaluating N samples brings 12 bytes per image to the host, plus the
fp32 images of the samples the grids show -- not 4 * S * S bytes for every sample.  Real images are decoded and resized by
the loader's helper, normalised on the device and counted by ``siggan_image_stats``.  FID / LPIPS are reported as not
computed (utils/metrics.py of this package).

Beyond the reference: ``--verifier_checkpoint PATH`` adds a Frechet distance between the real and the generated images in
the embedding space of the Siamese verifier (signature_verifier_eval), the FID construction over a network trained here.
Every generated batch's bytes go through ``embed_u8`` into an fp64 accumulator while they are still on the device
(utils/frechet.py), the real images take the same route, and dim * (dim + 1) doubles per set reach the host.
``--verifier_neighbors K`` (with ``--verifier_checkpoint`` and ``--real_dir``) adds what one distance cannot say: improved
precision / recall, density / coverage and the distance from every generated sample to its nearest real one, against the
real set's own leave-one-out distances -- the memorisation check.  The embeddings of both sets are then also kept in a
device buffer, and exact fp64 k-nearest-neighbour queries run there (utils/neighbors.py); k-lists and counts reach the
host.  ``--verifier_kid [PERMUTATIONS]`` (with ``--verifier_checkpoint`` and ``--real_dir``) adds the report key
``verifier_two_sample``: the Kernel Inception Distance (unbiased MMD^2 under the cubic polynomial kernel, mean and standard
deviation over 100 subsets) and a permutation test of the RBF-kernel MMD^2 with its p-value -- can the generated set be told
from the real one, and by more than chance at this sample size?  The embeddings are kept as for ``--verifier_neighbors``;
fp64 quadratic forms of the implicit kernel matrix run on the device (utils/twosample.py), three numbers per subset or
permutation reach the host.  A 128x128 Generator's bytes are shrunk to the verifier's 64x64 on the device first (resize.py: Pillow's antialiased
bilinear filter, byte for byte what the reference's verifier transform makes of the written PNG), the real files are
decoded at 64x64 for the verifier, and the report says so in ``verifier_input_resize``.
``--strokes`` adds the report key ``stroke_geometry``: skeleton length, line ends, junction pixels and a histogram of local
pen widths of the generated images (and of the real ones, under the same condition as ``fragmentation``), from a thinning and
an exact distance map of the bytes already on the device (strokes.py); 23 counters per image reach the host.
``--shape`` adds the report key ``shape_attributes``: the ink moments of the generated images (and of the real ones, under the
same condition) -- mass, centre, second moments, slant, spread; mean, standard deviation and 5 / 50 / 95th percentiles of
each --, from exact integer sums of the bytes already on the device (shape.py); six integers per image reach the host.
Without the flags nothing changes: stdout, report keys and exit codes are the reference's."""
import argparse
import json
import sys
from datetime import datetime
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from .data_loader_signatures import FILL, SignatureDataset, normalize_lut
from .generator_vanilla_gan import Generator
from .resize import resize_f32, resize_u8
from .train_vanilla_gan_signatures import save_sample_grid
from .utils.inference import load_generator_and_config
from .utils.frechet import FeatureMoments, embedding_spread, frechet_distance
from .utils.metrics import (DTW_DIVERSITY_IMAGES, INCEPTION_AVAILABLE, LPIPS_AVAILABLE, SSIM_DIVERSITY_IMAGES,
                            calculate_dtw_diversity, calculate_dtw_nearest_real, calculate_fid, calculate_foreground_ratio,
                            calculate_lpips_diversity, calculate_ssim_diversity, calculate_ssim_nearest_real,
                            calculate_stroke_density, foreground_ratio_from_counts,
                            fragmentation_from_counters, shape_attributes_from_features, stroke_density_from_counts,
                            stroke_geometry_from_counters, two_sample_metrics, verifier_embedding_chunks)
from .utils.neighbors import manifold_metrics

THRESHOLD = 0.5          # the threshold compute_metrics passes to both statistics (evaluate_vanilla_gan_signatures.py:306,318)
VERIFIER_IMAGE_SIZE = 64
COMPONENT_THRESHOLD, COMPONENT_CONNECTIVITY = 128, 8      # --components: ink is byte < 128, 8-connected


class GeneratedSamples:
    """What generate_samples hands on: the per-image stroke counters of all N samples (``counts``, int (N, 3) against
    ``threshold``) and the fp32 images of the first ``len(images)`` of them (CPU, (K, 1, S, S) in [-1, 1]).  When the
    samples were also embedded on the way (generate_samples' ``embedding_sink``): ``embedding_stats``, the finished
    (n, mean, cov) of their embeddings, or ``embedding_error`` saying why there is none; ``embeddings``, the (N, E) fp32
    device buffer of a sink that keeps them."""

    def __init__(self, n: int, image_shape: Tuple[int, int, int], counts: np.ndarray, images: torch.Tensor, threshold: float,
                 embedding_stats: Optional[Tuple[int, np.ndarray, np.ndarray]] = None, embedding_error: Optional[str] = None,
                 embeddings: Optional[torch.Tensor] = None):
        self.n, self.image_shape, self.counts, self.images, self.threshold = n, tuple(image_shape), counts, images, threshold
        self.embedding_stats, self.embedding_error, self.embeddings = embedding_stats, embedding_error, embeddings

    def __len__(self) -> int:
        return self.n

    @property
    def shape(self) -> Tuple[int, ...]:
        return (self.n,) + self.image_shape


def load_generator_from_checkpoint(checkpoint_path: Path, device: torch.device) -> Tuple[Generator, Dict[str, Any]]:
    """(Generator in eval mode, the checkpoint's config dict).  Safe loader only (utils.inference)."""
    checkpoint_path = Path(checkpoint_path)
    if not checkpoint_path.exists():
        raise FileNotFoundError(f"Checkpoint not found: {checkpoint_path}")
    print(f"Loading checkpoint from: {checkpoint_path}")
    generator, latent_dim, config = load_generator_and_config(str(checkpoint_path), device)
    print("Generator loaded successfully:")
    print(f"  - Latent dim: {latent_dim}")
    print(f"  - Image size: {generator.output_size}x{generator.output_size}")
    print(f"  - Epoch trained: {config.get('current_epoch', 'N/A')}")
    return generator, config


class EmbeddingSink:
    """One image set on its way into the verifier's embedding space: ``update`` embeds a batch (uint8 (B, 64, 64) or fp32
    (B, 1, 64, 64), on the device) and adds the embeddings to an fp64 accumulator there; ``finish`` -> (n, mean, cov).
    ``keep``: the embeddings also stay, and ``embeddings`` hands them on as one (n, E) fp32 device buffer.  ``resize``: uint8
    batches of another size (the 128x128 Generator's) go through resize.resize_u8 first -- Pillow's antialiased bilinear
    filter on the device, what the reference's verifier transform does to a written file."""

    def __init__(self, model, keep: bool = False, resize: bool = False) -> None:
        self.model, self.resize = model, bool(resize)
        self.moments = FeatureMoments(model.embedding_dim, next(model.parameters()).device)
        self.kept: Optional[List[torch.Tensor]] = [] if keep else None

    def update(self, images: torch.Tensor) -> None:
        if self.resize and tuple(images.shape[-2:]) != (VERIFIER_IMAGE_SIZE,) * 2:
            # (fp32 images of another size: the same map without the byte roundings -- main() never sends any, it hands
            # the real files over decoded at 64x64)
            images = (resize_u8 if images.dtype == torch.uint8 else resize_f32)(images.contiguous(), VERIFIER_IMAGE_SIZE)
        for emb in verifier_embedding_chunks(images, self.model):
            self.moments.update(emb)
            if self.kept is not None:
                self.kept.append(emb)

    def embeddings(self) -> Optional[torch.Tensor]:
        if not self.kept:
            return None
        return torch.cat(self.kept, dim=0).contiguous()

    def finish(self) -> Tuple[int, np.ndarray, np.ndarray]:
        try:
            return self.moments.finish()
        finally:
            self.moments.close()


class VerifierFeatures:
    """The Siamese verifier behind ``--verifier_checkpoint``: ``model`` (signature_verifier_eval.load_model), or ``error``
    saying why the Frechet distance cannot be computed with it -- the report records that, the evaluation goes on.
    ``input_resize``: None for a 64x64 Generator; for another size the name of the resize the generated bytes take on the
    device before the verifier sees them (``verifier_input_resize`` in the report)."""

    def __init__(self, checkpoint: Path, device: torch.device, image_size: int, neighbors_k: Optional[int] = None,
                 keep_embeddings: bool = False) -> None:
        self.checkpoint, self.model, self.error = str(checkpoint), None, None
        self.neighbors_k = neighbors_k                          # --verifier_neighbors: the sinks keep their embeddings
        self.keep_embeddings = bool(keep_embeddings)            # --verifier_kid: likewise
        self.input_resize = (None if image_size == VERIFIER_IMAGE_SIZE
                             else f"pillow_bilinear_{image_size}_to_{VERIFIER_IMAGE_SIZE}")
        try:
            from .signature_verifier_eval import load_model
            self.model, _ = load_model(self.checkpoint, device)
        except Exception as e:                                  # noqa: BLE001 -- recorded like fid_error
            self.error = f"could not load the verifier checkpoint: {e}"

    def sink(self) -> Optional[EmbeddingSink]:
        if self.model is None:
            return None
        return EmbeddingSink(self.model, keep=self.neighbors_k is not None or self.keep_embeddings,
                             resize=self.input_resize is not None)


class ComponentSink:
    """Collects the component counters (components.component_stats, int32 (B, 9)) of every uint8 batch it is shown while the
    batch is on the device; ``counters()`` brings all of them to the host at once.  ``min_area`` None: resolved to
    components.default_min_area of the first batch's size."""

    def __init__(self, min_area: Optional[int] = None, threshold: int = COMPONENT_THRESHOLD,
                 connectivity: int = COMPONENT_CONNECTIVITY) -> None:
        self.min_area, self.threshold, self.connectivity, self.parts = min_area, threshold, connectivity, []

    def update(self, u8: torch.Tensor) -> None:
        from .components import component_stats, default_min_area
        if self.min_area is None:
            self.min_area = default_min_area(u8.shape[-2], u8.shape[-1])
        self.parts.append(component_stats(u8.contiguous(), self.threshold, self.connectivity, self.min_area))

    def counters(self) -> np.ndarray:
        return torch.cat(self.parts).cpu().numpy() if self.parts else np.zeros((0, 9), np.int32)


class StrokeSink:
    """Collects the stroke counters (strokes.stroke_stats, int32 (B, 23)) of every uint8 batch it is shown while the batch is on
    the device (--strokes); ``counters()`` brings all of them to the host at once."""

    def __init__(self, threshold: int = COMPONENT_THRESHOLD) -> None:
        self.threshold, self.parts = threshold, []

    def update(self, u8: torch.Tensor) -> None:
        from .strokes import stroke_stats
        self.parts.append(stroke_stats(u8.contiguous(), self.threshold))

    def counters(self) -> np.ndarray:
        return torch.cat(self.parts).cpu().numpy() if self.parts else np.zeros((0, 23), np.int32)


class ShapeSink:
    """Collects the six integer moment sums (shape.shape_sums_u8, int64 (B, 6)) of every uint8 batch it is shown while the batch
    is on the device (--shape); ``features()`` brings them to the host at once and makes the (N, 8) features of them."""

    def __init__(self) -> None:
        self.parts, self.size = [], None

    def update(self, u8: torch.Tensor) -> None:
        from .shape import shape_sums_u8
        self.size = int(u8.shape[-1])
        self.parts.append(shape_sums_u8(u8.contiguous()))

    def features(self) -> np.ndarray:
        from .shape import features_from_sums
        return features_from_sums(torch.cat(self.parts).cpu().numpy(), self.size)


class SsimSink:
    """Keeps the bytes of every uint8 batch it is shown, on the device (--ssim, --dtw): the comparisons between images need the
    whole set at once.  ``images()``: all of them, uint8 (N, H, W)."""

    def __init__(self) -> None:
        self.parts = []

    def update(self, u8: torch.Tensor) -> None:
        self.parts.append(u8.reshape(u8.shape[0], u8.shape[-2], u8.shape[-1]).clone())

    def images(self) -> Optional[torch.Tensor]:
        return torch.cat(self.parts).contiguous() if self.parts else None


@torch.no_grad()
def generate_samples(generator: Generator, n_samples: int, latent_dim: int, device: torch.device, batch_size: int = 64,
                     keep_images: Optional[int] = None, threshold: float = THRESHOLD,
                     embedding_sink: Optional[EmbeddingSink] = None,
                     component_sink: Optional[ComponentSink] = None, ssim_sink: Optional[SsimSink] = None,
                     stroke_sink: Optional[StrokeSink] = None, shape_sink: Optional[ShapeSink] = None) -> GeneratedSamples:
    """N samples, z = torch.randn per batch as the reference draws it (so a seed means the same).  ``keep_images``: how
    many leading samples to bring back as fp32 images (None: all, what the reference returns).  ``embedding_sink``: receives
    every batch's uint8 tensor while it is on the device; its finished statistics travel in the result.  ``component_sink``:
    is shown the same bytes and keeps their component counters; ``ssim_sink`` keeps the bytes themselves; ``stroke_sink``
    keeps their stroke counters, ``shape_sink`` their moment sums."""
    generator.eval()
    eng = generator._require_engine()
    keep = n_samples if keep_images is None else max(0, min(int(keep_images), n_samples))
    n_batches = (n_samples + batch_size - 1) // batch_size
    counts, images = [], []
    print(f"Generating {n_samples} samples...")
    for i in range(n_batches):
        b = min(batch_size, n_samples - i * batch_size)
        z = torch.randn(b, latent_dim, device=device)
        want = min(b, keep - i * batch_size)
        if want > 0:
            u8, st, img = eng.g_generate_u8(z, threshold=threshold, want_f32=True)
            images.append(img[:want].cpu())
        else:
            u8, st = eng.g_generate_u8(z, threshold=threshold)
        counts.append(st)
        if embedding_sink is not None:
            embedding_sink.update(u8)
        if component_sink is not None:
            component_sink.update(u8)
        if ssim_sink is not None:
            ssim_sink.update(u8)
        if stroke_sink is not None:
            stroke_sink.update(u8)
        if shape_sink is not None:
            shape_sink.update(u8)
        if (i + 1) % 10 == 0 or i == n_batches - 1:
            print(f"  Generated {min((i + 1) * batch_size, n_samples)}/{n_samples} samples")
    s = generator.output_size
    kept = torch.cat(images, dim=0) if images else torch.empty(0, 1, s, s)
    all_counts = torch.cat(counts, dim=0).cpu().numpy() if counts else np.zeros((0, 3), np.int32)
    stats, error, embeddings = None, None, None
    if embedding_sink is not None:
        embeddings = embedding_sink.embeddings()
        try:
            stats = embedding_sink.finish()
        except ValueError as e:                                 # fewer than 2 samples: the report says so
            error = str(e)
    return GeneratedSamples(n_samples, (1, s, s), all_counts, kept, threshold, stats, error, embeddings)


def load_real_images(real_dir: Path, n_images: int, image_size: int, device: torch.device,
                     verifier_size: Optional[int] = None, component_sink: Optional[ComponentSink] = None,
                     ssim_sink: Optional[SsimSink] = None, stroke_sink: Optional[StrokeSink] = None,
                     shape_sink: Optional[ShapeSink] = None):
    """Up to ``n_images`` files of ``real_dir`` as (N, 1, S, S) fp32 in [-1, 1] ON THE DEVICE: decoded and resized by the
    loader's helper (PIL -> 'L' -> bilinear), normalised by its byte table in the input-pipeline kernel.
    ``verifier_size``: -> (that tensor, the SAME files decoded at verifier_size as uint8 (N, V, V) on the device) -- what the
    reference's verifier sees of a real file, which it resizes from the file and not from a 128x128 copy.
    ``component_sink`` / ``ssim_sink`` / ``stroke_sink`` / ``shape_sink``: are shown the decoded BYTES (the cache the normalisation reads), not
    a re-quantised fp32 copy."""
    from . import _lib
    real_dir = Path(real_dir)
    if not real_dir.exists():
        raise FileNotFoundError(f"Real images directory not found: {real_dir}")
    ds = SignatureDataset(real_dir)
    if len(ds) == 0:
        raise ValueError(f"No images found in {real_dir}")
    picks = list(range(len(ds)))
    if len(picks) > n_images:
        picks = [int(i) for i in np.random.choice(len(picks), n_images, replace=False)]
    print(f"Loading {len(picks)} real images from {real_dir}")
    decoded, small = [], []
    for i in picks:
        arr = ds.decode(i, image_size)
        if arr is None:
            print(f"  Warning: Failed to load {ds.get_image_path(i)}: unreadable image")
        else:
            decoded.append(arr)
            if verifier_size is not None:
                small.append(ds.decode(i, verifier_size))
    if not decoded:
        raise ValueError("No images could be loaded successfully")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("real images are normalised and counted on a ROCm device ('cuda:N'); there is no CPU path")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    n = len(decoded)
    cache = torch.from_numpy(np.stack(decoded)).to(dev)
    if component_sink is not None:
        component_sink.update(cache)
    if ssim_sink is not None:
        ssim_sink.update(cache)
    if stroke_sink is not None:
        stroke_sink.update(cache)
    if shape_sink is not None:
        shape_sink.update(cache)
    index = torch.arange(n, dtype=torch.int32, device=dev)
    lut = normalize_lut((-1.0, 1.0)).to(dev)
    out = torch.empty(n, 1, image_size, image_size, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().siggan_augment_batch(dev.index, cache.data_ptr(), n, index.data_ptr(), None, None, lut.data_ptr(),
                                                out.data_ptr(), n, image_size, 0, FILL,
                                                torch.cuda.current_stream(dev).cuda_stream))
    if verifier_size is not None:
        return out, torch.from_numpy(np.stack(small)).to(dev)
    return out


def create_sample_grids(samples, output_dir: Path, n_grids: int = 3, grid_size: int = 64) -> List[Path]:
    """Up to ``n_grids`` PNG grids of ``grid_size`` samples each (the trainer's grid writer); ``samples``: an (N, C, H, W)
    tensor or a GeneratedSamples (its kept images)."""
    images = samples.images if isinstance(samples, GeneratedSamples) else samples
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
    saved: List[Path] = []
    for i in range(n_grids):
        lo = i * grid_size
        if lo >= len(images):
            break
        chunk = images[lo:min(lo + grid_size, len(images))]
        path = output_dir / f"sample_grid_{stamp}_{i + 1}.png"
        save_sample_grid(chunk, path, nrow=int(np.sqrt(len(chunk))))
        saved.append(path)
        print(f"  Saved grid: {path}")
    return saved


def _stroke(images) -> Dict[str, float]:
    if isinstance(images, GeneratedSamples):
        return stroke_density_from_counts(images.counts, int(np.prod(images.image_shape)))
    return calculate_stroke_density(images, threshold=THRESHOLD)


def _foreground(images) -> Dict[str, Any]:
    if isinstance(images, GeneratedSamples):
        return foreground_ratio_from_counts(images.counts, int(np.prod(images.image_shape)))
    return calculate_foreground_ratio(images, threshold=THRESHOLD)


def _verifier_frechet(metrics: Dict[str, Any], fake_images, real_images: Optional[torch.Tensor],
                      verifier: VerifierFeatures) -> Optional[torch.Tensor]:
    """The ``verifier_*`` keys of the report; any failure is recorded as ``verifier_frechet_error``, like ``fid_error``.
    ``real_images``: what the verifier is to see of the real set -- fp32 (N, 1, 64, 64) or uint8 (N, 64, 64).
    -> the real images' embeddings when the sink kept them (``--verifier_neighbors``, ``--verifier_kid``), else None."""
    metrics["verifier_checkpoint"] = verifier.checkpoint
    metrics["verifier_input_resize"] = verifier.input_resize
    real_embeddings = None
    print("Computing verifier Frechet distance...")
    try:
        if verifier.error:
            raise ValueError(verifier.error)
        if real_images is None:
            raise ValueError("no real images provided")
        fake_stats = getattr(fake_images, "embedding_stats", None)
        if fake_stats is None:
            raise ValueError(getattr(fake_images, "embedding_error", None) or "the generated samples were not embedded")
        sink = verifier.sink()
        sink.update(real_images)
        real_embeddings = sink.embeddings()
        (_, mu_r, cov_r), (_, mu_f, cov_f) = sink.finish(), fake_stats
        metrics["verifier_frechet_distance"] = frechet_distance(mu_r, cov_r, mu_f, cov_f)
        metrics["verifier_embedding_spread"] = {"generated": embedding_spread(cov_f), "real": embedding_spread(cov_r)}
        print(f"  Verifier Frechet Distance: {metrics['verifier_frechet_distance']:.4f}")
    except Exception as e:                                      # noqa: BLE001 -- the report records any failure
        print(f"  Skipping verifier Frechet distance: {e}")
        metrics["verifier_frechet_distance"], metrics["verifier_frechet_error"] = None, str(e)
    return real_embeddings


NEIGHBOR_KEYS = ("verifier_precision", "verifier_recall", "verifier_density", "verifier_coverage", "verifier_nearest_real")


def _verifier_neighbors(metrics: Dict[str, Any], fake_images, real_embeddings: Optional[torch.Tensor],
                        verifier: Optional[VerifierFeatures], k: int) -> None:
    """The keys ``--verifier_neighbors K`` adds (NEIGHBOR_KEYS, ``verifier_neighbors_k``), from the embeddings both sinks
    kept; any failure is recorded as ``verifier_neighbors_error`` and the five figures are None."""
    metrics["verifier_neighbors_k"] = k
    print("Computing verifier precision / recall and nearest-real distances...")
    try:
        if verifier is None:
            raise ValueError("--verifier_neighbors needs --verifier_checkpoint")
        if verifier.error:
            raise ValueError(verifier.error)
        fake_embeddings = getattr(fake_images, "embeddings", None)
        if fake_embeddings is None:
            raise ValueError("the generated samples were not embedded")
        if real_embeddings is None:
            raise ValueError(metrics.get("verifier_frechet_error") or "no real images provided")
        m = manifold_metrics(real_embeddings, fake_embeddings, k)
        for key in NEIGHBOR_KEYS:
            metrics[key] = m[key[len("verifier_"):]]
        nr = m["nearest_real"]
        print(f"  Verifier Precision: {m['precision']:.4f}, Recall: {m['recall']:.4f}, "
              f"Density: {m['density']:.4f}, Coverage: {m['coverage']:.4f}")
        print(f"  Nearest real - Median: {nr['median']:.4f} (real leave-one-out: {nr['real_loo_median']:.4f})")
    except Exception as e:                                      # noqa: BLE001 -- the report records any failure
        print(f"  Skipping verifier precision / recall: {e}")
        for key in NEIGHBOR_KEYS:
            metrics[key] = None
        metrics["verifier_neighbors_error"] = str(e)


TWO_SAMPLE_SEED = 0      # the subsets and permutations of --verifier_kid do not move with --seed: a p-value is comparable across runs


def _verifier_two_sample(metrics: Dict[str, Any], fake_images, real_embeddings: Optional[torch.Tensor],
                         verifier: Optional[VerifierFeatures], permutations: int) -> None:
    """The key ``--verifier_kid`` adds, ``verifier_two_sample`` = {kid, mmd_test, n_real, n_generated}, from the embeddings
    both sinks kept; any failure is recorded as ``verifier_two_sample_error`` and the key is None."""
    print("Computing verifier KID and the MMD permutation test...")
    try:
        if verifier is None:
            raise ValueError("--verifier_kid needs --verifier_checkpoint")
        if verifier.error:
            raise ValueError(verifier.error)
        fake_embeddings = getattr(fake_images, "embeddings", None)
        if fake_embeddings is None:
            raise ValueError("the generated samples were not embedded")
        if real_embeddings is None:
            raise ValueError(metrics.get("verifier_frechet_error") or "no real images provided")
        m = metrics["verifier_two_sample"] = two_sample_metrics(real_embeddings, fake_embeddings, permutations, seed=TWO_SAMPLE_SEED)
        print(f"  Verifier KID: {m['kid']['kid_mean']:.6f} +- {m['kid']['kid_std']:.6f}, "
              f"MMD^2: {m['mmd_test']['mmd2']:.6f} (p = {m['mmd_test']['p_value']:.4f})")
    except Exception as e:                                      # noqa: BLE001 -- the report records any failure
        print(f"  Skipping verifier KID / MMD test: {e}")
        metrics["verifier_two_sample"], metrics["verifier_two_sample_error"] = None, str(e)


MODES_SEED = 0           # like TWO_SAMPLE_SEED: the split, the seeding and so the bins of --modes do not move with --seed


def _mode_coverage(metrics: Dict[str, Any], fake_images, real_embeddings: Optional[torch.Tensor],
                   verifier: Optional[VerifierFeatures], request: Dict[str, Any]) -> None:
    """The key ``--modes`` adds, ``mode_coverage`` = utils.modes.mode_coverage's dictionary plus feature_space and feature_dim.
    ``request``: {k (None: utils.modes.default_k), generated, real (the SsimSinks that kept the bytes; unused with a verifier)}.
    With a verifier the rows are the embeddings both sinks kept ('verifier'), else utils.modes.pixel_features of the bytes
    ('pixels/4').  Any failure is recorded as ``mode_coverage_error`` and the key is None."""
    from .utils.modes import mode_coverage, pixel_features
    print("Computing mode coverage (k-means bins, NDB and JS divergence)...")
    try:
        if verifier is not None:
            if verifier.error:
                raise ValueError(verifier.error)
            fake, real, space = getattr(fake_images, "embeddings", None), real_embeddings, "verifier"
            if fake is None:
                raise ValueError("the generated samples were not embedded")
            if real is None:
                raise ValueError(metrics.get("verifier_frechet_error") or "no real images provided")
        else:
            real_u8 = request["real"].images()
            if real_u8 is None:
                raise ValueError("no real images provided")
            fake, real, space = pixel_features(request["generated"].images()), pixel_features(real_u8), "pixels/4"
        m = mode_coverage(real, fake, k=request["k"], seed=MODES_SEED)
        m["feature_space"], m["feature_dim"] = space, int(real.shape[1])
        metrics["mode_coverage"] = m
        print(f"  NDB / K: {m['generated_vs_real']['ndb_over_k']:.4f} over {m['k']} bins ({space}), JS divergence: "
              f"{m['generated_vs_real']['js_divergence']:.4f}")
    except Exception as e:                                      # noqa: BLE001 -- the report records any failure
        print(f"  Skipping mode coverage: {e}")
        metrics["mode_coverage"], metrics["mode_coverage_error"] = None, str(e)


def compute_metrics(fake_images, real_images: Optional[torch.Tensor], device: torch.device,
                    verifier: Optional[VerifierFeatures] = None, neighbors_k: Optional[int] = None,
                    verifier_real: Optional[torch.Tensor] = None, fragmentation: Optional[Dict[str, Any]] = None,
                    pixel_similarity: Optional[Dict[str, Any]] = None,
                    stroke_geometry: Optional[Dict[str, Any]] = None,
                    shape_attributes: Optional[Dict[str, Any]] = None,
                    kid_permutations: Optional[int] = None,
                    elastic_similarity: Optional[Dict[str, Any]] = None,
                    modes: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """The report's ``metrics`` dictionary.  ``fake_images``: a GeneratedSamples (its counters are used) or a tensor.
    ``verifier``: add the Frechet distance over its embeddings (the ``verifier_*`` keys; none without it).
    ``verifier_real``: the real set as the verifier is to see it when that is not ``real_images`` (a 128x128 Generator: the
    files decoded at 64x64, load_real_images' second result); the pixel-space metrics keep ``real_images``.
    ``neighbors_k``: add precision / recall, density / coverage and the nearest-real distances at that k.
    ``fragmentation``: the finished ``fragmentation`` block (fragmentation_block), added as it is; no key without it.
    ``pixel_similarity``: likewise the finished ``pixel_similarity`` block (pixel_similarity_block); ``stroke_geometry``:
    likewise the finished ``stroke_geometry`` block (stroke_geometry_block); ``shape_attributes``: likewise the finished
    ``shape_attributes`` block (shape_attributes_block).  ``kid_permutations``: add ``verifier_two_sample``, the KID and
    the MMD permutation test with that many permutations.  ``elastic_similarity``: the finished ``elastic_similarity`` block
    (elastic_similarity_block), added as it is; no key without it.  ``modes``: add ``mode_coverage`` (_mode_coverage's request)."""
    metrics: Dict[str, Any] = {"n_samples": len(fake_images), "image_shape": list(fake_images.shape[1:]),
                               "metrics_computed_at": datetime.now().isoformat()}
    if real_images is not None and INCEPTION_AVAILABLE:
        print("Computing FID score...")
        try:
            metrics["fid_score"] = calculate_fid(real_images, getattr(fake_images, "images", fake_images), device)
            print(f"  FID Score: {metrics['fid_score']:.4f}")
        except Exception as e:                                  # noqa: BLE001 -- the report records any failure
            print(f"  Warning: FID computation failed: {e}")
            metrics["fid_score"], metrics["fid_error"] = None, str(e)
    elif not INCEPTION_AVAILABLE:
        print("  Skipping FID: torchvision not available")
        metrics["fid_score"], metrics["fid_error"] = None, "torchvision not available"
    else:
        print("  Skipping FID: no real images provided")
        metrics["fid_score"], metrics["fid_error"] = None, "no real images provided"

    if LPIPS_AVAILABLE:
        print("Computing LPIPS diversity...")
        try:
            pool = getattr(fake_images, "images", fake_images)
            metrics["lpips_diversity"] = calculate_lpips_diversity([pool[i] for i in range(min(100, len(pool)))], device)
            print(f"  LPIPS Diversity: {metrics['lpips_diversity']:.4f}")
        except Exception as e:                                  # noqa: BLE001
            print(f"  Warning: LPIPS computation failed: {e}")
            metrics["lpips_diversity"], metrics["lpips_error"] = None, str(e)
    else:
        print("  Skipping LPIPS: lpips package not available")
        metrics["lpips_diversity"], metrics["lpips_error"] = None, "lpips package not available"

    real_embeddings = None
    if verifier is not None:
        real_embeddings = _verifier_frechet(metrics, fake_images, real_images if verifier_real is None else verifier_real, verifier)
    if neighbors_k is not None:
        _verifier_neighbors(metrics, fake_images, real_embeddings, verifier, neighbors_k)
    if kid_permutations is not None:
        _verifier_two_sample(metrics, fake_images, real_embeddings, verifier, kid_permutations)
    if modes is not None:
        _mode_coverage(metrics, fake_images, real_embeddings, verifier, modes)

    print("Computing stroke density distribution...")
    try:
        sd = metrics["stroke_density"] = _stroke(fake_images)
        print(f"  Stroke Density - Mean: {sd['mean']:.4f}, Std: {sd['std']:.4f}")
    except Exception as e:                                      # noqa: BLE001
        print(f"  Warning: Stroke density computation failed: {e}")
        metrics["stroke_density"], metrics["stroke_density_error"] = None, str(e)
    print("Computing foreground ratio statistics...")
    try:
        fr = metrics["foreground_ratio"] = _foreground(fake_images)
        print(f"  Foreground Ratio - Mean: {fr['mean']:.4f}, Std: {fr['std']:.4f}")
    except Exception as e:                                      # noqa: BLE001
        print(f"  Warning: Foreground ratio computation failed: {e}")
        metrics["foreground_ratio"], metrics["foreground_ratio_error"] = None, str(e)

    if real_images is not None:
        print("Computing real image statistics for comparison...")
        try:
            rs, rf = _stroke(real_images), _foreground(real_images)
            metrics["real_stroke_density"], metrics["real_foreground_ratio"] = rs, rf
            print(f"  Real Stroke Density - Mean: {rs['mean']:.4f}")
            print(f"  Real Foreground Ratio - Mean: {rf['mean']:.4f}")
        except Exception as e:                                  # noqa: BLE001
            print(f"  Warning: Real image statistics failed: {e}")
    if fragmentation is not None:
        metrics["fragmentation"] = fragmentation
        g = fragmentation["generated"]
        print(f"  Ink components per image - Mean: {g['components_mean']:.2f}, speckle ink ratio: {g['speckle_ink_ratio']:.4f}")
    if pixel_similarity is not None:
        metrics["pixel_similarity"] = pixel_similarity
        print(f"  SSIM diversity (1 - mean pairwise SSIM): {_fmt(pixel_similarity['generated_diversity']['all_pairs']['diversity'])}")
    if elastic_similarity is not None:
        metrics["elastic_similarity"] = elastic_similarity
        print(f"  DTW diversity (mean pairwise distance per column): {_fmt(elastic_similarity['generated_diversity']['all_pairs']['diversity'])}")
    if stroke_geometry is not None:
        metrics["stroke_geometry"] = stroke_geometry
        g = stroke_geometry["generated"]
        print(f"  Pen width along the skeleton - Mean: {_fmt(g['mean_width'])}, skeleton length: {_fmt(g['skeleton_length']['mean'])}")
    if shape_attributes is not None:
        metrics["shape_attributes"] = shape_attributes
        print(f"  Shape attributes - {_shape_line(shape_attributes['generated'])}")
    return metrics


def _fmt(v: Optional[float]) -> str:
    return "n/a" if v is None else format(v, ".4f")


def pixel_similarity_block(generated: SsimSink, real: Optional[SsimSink] = None) -> Dict[str, Any]:
    """The report's ``pixel_similarity`` key (--ssim): {window, generated_diversity, and with a real set real_diversity and
    nearest_real}.  Diversity: utils.metrics.calculate_ssim_diversity over at most the set's first 512 images; nearest_real:
    calculate_ssim_nearest_real over every generated and every real image.  Each set is prepared once."""
    from .ssim import WINDOW_SIGMA, WINDOW_TAPS, SsimSet, window
    fake = SsimSet(generated.images())
    block: Dict[str, Any] = {"window": {"taps": WINDOW_TAPS, "sigma": WINDOW_SIGMA, "weights": [float(v) for v in window()],
                                        "dynamic_range": 255, "valid_positions_only": True},
                             "diversity_images": SSIM_DIVERSITY_IMAGES,
                             "generated_diversity": calculate_ssim_diversity(fake)}
    if real is not None and real.parts:
        true = SsimSet(real.images())
        block["real_diversity"] = calculate_ssim_diversity(true)
        block["nearest_real"] = calculate_ssim_nearest_real(fake, true)
    return block


def elastic_similarity_block(generated: SsimSink, real: Optional[SsimSink] = None, band: Optional[int] = None,
                             threshold: int = 128) -> Dict[str, Any]:
    """The report's ``elastic_similarity`` key (--dtw): {band, threshold, generated_diversity, and with a real set real_diversity
    and nearest_real}, banded DTW distances between column profiles, per column.  Diversity:
    utils.metrics.calculate_dtw_diversity over at most the set's first 512 images; nearest_real: calculate_dtw_nearest_real over
    every generated and every real image.  ``band`` None: dtw.default_band of the width.  Each set is profiled once."""
    from .dtw import DtwSet, check_band
    fake = DtwSet(generated.images(), threshold)
    band = check_band(band, fake.w)
    block: Dict[str, Any] = {"band": band, "threshold": threshold, "diversity_images": DTW_DIVERSITY_IMAGES,
                             "generated_diversity": calculate_dtw_diversity(fake, band)}
    if real is not None and real.parts:
        true = DtwSet(real.images(), threshold)
        block["real_diversity"] = calculate_dtw_diversity(true, band)
        block["nearest_real"] = calculate_dtw_nearest_real(fake, true, band)
    return block


def _shape_line(d: Dict[str, Any]) -> str:
    mean = lambda name: _fmt(None if d[name] is None else d[name]["mean"])                  # noqa: E731
    return (f"slant {mean('slant')} (negative leans right), spread {mean('spread')}, mass {mean('mass')}, centre "
            f"({mean('cx')}, {mean('cy')}), {d['empty']} empty")


def shape_attributes_block(generated: ShapeSink, real: Optional[ShapeSink] = None) -> Dict[str, Any]:
    """The report's ``shape_attributes`` key (--shape): {generated, real (only when a real set was measured)}, each side a
    utils.metrics.shape_attributes_from_features dictionary: per ink moment (shape.FEATURES) the mean, standard deviation
    and 5th / 50th / 95th percentiles over the set, from the exact integer sums of the bytes."""
    block: Dict[str, Any] = {"generated": shape_attributes_from_features(generated.features())}
    if real is not None and real.parts:
        block["real"] = shape_attributes_from_features(real.features())
    return block


def stroke_geometry_block(generated: StrokeSink, real: Optional[StrokeSink] = None) -> Dict[str, Any]:
    """The report's ``stroke_geometry`` key (--strokes): {threshold, generated, real (only when a real set was measured)}, each
    side a utils.metrics.stroke_geometry_from_counters dictionary."""
    block: Dict[str, Any] = {"threshold": generated.threshold, "generated": stroke_geometry_from_counters(generated.counters())}
    if real is not None and real.parts:
        block["real"] = stroke_geometry_from_counters(real.counters())
    return block


def fragmentation_block(generated: ComponentSink, real: Optional[ComponentSink] = None) -> Dict[str, Any]:
    """The report's ``fragmentation`` key: {generated, real (only when a real set was counted), threshold, connectivity,
    min_area}, each side a utils.metrics.fragmentation_from_counters dictionary."""
    block: Dict[str, Any] = {"generated": fragmentation_from_counters(generated.counters())}
    if real is not None and real.parts:
        block["real"] = fragmentation_from_counters(real.counters())
    block.update(threshold=generated.threshold, connectivity=generated.connectivity, min_area=generated.min_area)
    return block


def save_evaluation_report(metrics: Dict[str, Any], config: Dict[str, Any], output_dir: Path, checkpoint_path: Path,
                           grid_paths: List[Path]) -> Path:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    # the verifier's distance joins the summary of a report that has it; a report made without the flag keeps its keys
    extra = {key: metrics[key] for key in ("verifier_frechet_distance", "verifier_precision", "verifier_recall") if key in metrics}
    report = {
        "evaluation_info": {"checkpoint": str(checkpoint_path), "evaluation_timestamp": datetime.now().isoformat(),
                            "sample_grids": [str(p) for p in grid_paths]},
        "model_config": config,
        "metrics": metrics,
        "summary": {"fid_score": metrics.get("fid_score"), "lpips_diversity": metrics.get("lpips_diversity"),
                    "stroke_density_mean": (metrics.get("stroke_density") or {}).get("mean"),
                    "foreground_ratio_mean": (metrics.get("foreground_ratio") or {}).get("mean"),
                    "n_samples_evaluated": metrics.get("n_samples"), **extra},
    }
    path = output_dir / f"evaluation_report_{datetime.now().strftime('%Y%m%d_%H%M%S')}.json"
    with open(path, "w") as f:
        json.dump(report, f, indent=2, default=str)
    print(f"\nEvaluation report saved to: {path}")
    return path


def print_summary(metrics: Dict[str, Any]) -> None:
    bar = "=" * 60
    print("\n" + bar + "\nEVALUATION SUMMARY\n" + bar)
    print(f"\nSamples Evaluated: {metrics.get('n_samples', 'N/A')}")
    print(f"Image Shape: {metrics.get('image_shape', 'N/A')}")
    print("\n--- Quality Metrics ---")
    fid, lp = metrics.get("fid_score"), metrics.get("lpips_diversity")
    print(f"FID Score: {fid:.4f} (lower is better)" if fid is not None
          else f"FID Score: Not computed - {metrics.get('fid_error', 'unknown reason')}")
    print(f"LPIPS Diversity: {lp:.4f} (higher = more diverse)" if lp is not None
          else f"LPIPS Diversity: Not computed - {metrics.get('lpips_error', 'unknown reason')}")
    if "pixel_similarity" in metrics:
        ps = metrics["pixel_similarity"]
        g = ps["generated_diversity"]
        line = (f"SSIM Diversity: {_fmt(g['all_pairs']['diversity'])} (1 - mean pairwise SSIM over {g['n']} images, higher = more "
                f"diverse; {_fmt(g['lpips_pairs']['diversity'])} on the LPIPS pair set)")
        if "real_diversity" in ps:
            line += f"; real set: {_fmt(ps['real_diversity']['all_pairs']['diversity'])}"
        print(line)
        if "nearest_real" in ps:
            nr = ps["nearest_real"]
            print(f"SSIM to the nearest real image: median {nr['median']:.4f}, max {nr['max']:.4f} (real leave-one-out median "
                  f"{_fmt(nr['real_loo_median'])}, excess {_fmt(nr['excess_median'])}; clearly positive = memorisation warning)")
    if "elastic_similarity" in metrics:
        es = metrics["elastic_similarity"]
        g = es["generated_diversity"]
        line = (f"DTW Diversity: {_fmt(g['all_pairs']['diversity'])} (mean pairwise column-profile DTW distance per column over {g['n']} "
                f"images, band {es['band']}, higher = more diverse; {_fmt(g['lpips_pairs']['diversity'])} on the LPIPS pair set)")
        if "real_diversity" in es:
            line += f"; real set: {_fmt(es['real_diversity']['all_pairs']['diversity'])}"
        print(line)
        if "nearest_real" in es:
            nr = es["nearest_real"]
            print(f"DTW to the nearest real image: median {nr['median']:.4f}, min {nr['min']:.4f} per column (real leave-one-out median "
                  f"{_fmt(nr['real_loo_median'])}, excess {_fmt(nr['excess_median'])}; clearly positive = memorisation warning)")
    if "verifier_frechet_distance" in metrics:
        vfd = metrics["verifier_frechet_distance"]
        print(f"Verifier Frechet Distance: {vfd:.4f} (lower is better)" if vfd is not None
              else f"Verifier Frechet Distance: Not computed - {metrics.get('verifier_frechet_error', 'unknown reason')}")
    if "verifier_precision" in metrics:
        for label, key, hint in (("Precision", "verifier_precision", "generated samples inside the real manifold"),
                                 ("Recall", "verifier_recall", "real samples inside the generated manifold")):
            v = metrics[key]
            print(f"Verifier {label}: {v:.4f} ({hint}, k = {metrics.get('verifier_neighbors_k')})" if v is not None
                  else f"Verifier {label}: Not computed - {metrics.get('verifier_neighbors_error', 'unknown reason')}")
    if "verifier_two_sample" in metrics:
        ts = metrics["verifier_two_sample"]
        if ts is None:
            why = metrics.get("verifier_two_sample_error", "unknown reason")
            print(f"Verifier KID: Not computed - {why}")
            print(f"Verifier MMD test: Not computed - {why}")
        else:
            k, t = ts["kid"], ts["mmd_test"]
            print(f"Verifier KID: {k['kid_mean']:.6f} +- {k['kid_std']:.6f} ({k['subsets']} subsets of {k['subset_size']}, lower is "
                  f"better; full sets {k['kid_full']:.6f})")
            print(f"Verifier MMD^2 ({t['kind']}, gamma {t['gamma']:.4g}): {t['mmd2']:.6f}, p = {t['p_value']:.4f} over "
                  f"{t['permutations']} permutations (null 95% quantile {t['null_q95']:.6f}; small p = the sets can be told apart)")
    if "mode_coverage" in metrics:
        mc = metrics["mode_coverage"]
        if mc is None:
            why = metrics.get("mode_coverage_error", "unknown reason")
            print(f"Mode coverage (NDB): Not computed - {why}")
            print(f"Missing modes: Not computed - {why}")
        else:
            g, floor = mc["generated_vs_real"], mc["real_holdout_vs_real"]
            print(f"Mode coverage (NDB): {g['ndb']} of {mc['k']} bins differ, NDB / K {g['ndb_over_k']:.4f}, JS divergence "
                  f"{g['js_divergence']:.4f} ({mc['feature_space']}; real hold-out floor: "
                  + (f"NDB / K {floor['ndb_over_k']:.4f}, JS {floor['js_divergence']:.4f}" if floor is not None
                     else f"none - {mc['real_holdout_reason']}") + "; lower is better)")
            print(f"Missing modes: {len(g['missing_bins'])} bins hold no generated sample; most under-represented: "
                  + (", ".join(f"bin {e['bin']} (nearest real row {e['real_row']})" for e in mc["under_represented_examples"]) or "none"))
    print("\n--- Stroke Analysis ---")
    stroke = metrics.get("stroke_density")
    if stroke:
        print("Stroke Density:")
        print(f"  Mean: {stroke['mean']:.4f}")
        print(f"  Std:  {stroke['std']:.4f}")
        print(f"  Range: [{stroke['min']:.4f}, {stroke['max']:.4f}]")
    print("\n--- Foreground Analysis ---")
    fg = metrics.get("foreground_ratio")
    if fg:
        print("Foreground Ratio:")
        print(f"  Mean: {fg['mean']:.4f}")
        print(f"  Std:  {fg['std']:.4f}")
        if "percentiles" in fg:
            pc = fg["percentiles"]
            print(f"  Percentiles: 25%={pc['25']:.4f}, 50%={pc['50']:.4f}, 75%={pc['75']:.4f}")
    if "real_stroke_density" in metrics:
        print("\n--- Comparison with Real Images ---")
        rs, rf = metrics["real_stroke_density"], metrics.get("real_foreground_ratio", {})
        print(f"Real Stroke Density Mean: {rs['mean']:.4f} (Generated: {stroke['mean']:.4f})")
        if rf:
            print(f"Real Foreground Ratio Mean: {rf['mean']:.4f} (Generated: {fg['mean']:.4f})")
    if "fragmentation" in metrics:
        fr = metrics["fragmentation"]
        print(f"\n--- Fragmentation (ink components, min area {fr['min_area']} px, {fr['connectivity']}-connected) ---")
        for side in ("generated", "real"):
            if side in fr:
                d = fr[side]
                share = d["largest_component_share_mean"]
                print(f"{side.capitalize()}: {d['components_mean']:.2f} components per image (median {d['components_median']:.1f}), "
                      f"{d['small_components_mean']:.2f} specks, speckle ink ratio {d['speckle_ink_ratio']:.4f}, largest component share "
                      f"{'n/a' if share is None else format(share, '.4f')}, {d['empty_images']} empty")
    if "stroke_geometry" in metrics:
        sg = metrics["stroke_geometry"]
        print(f"\n--- Stroke geometry (skeleton and pen width, ink < {sg['threshold']}) ---")
        for side in ("generated", "real"):
            if side in sg:
                d = sg[side]
                print(f"{side.capitalize()}: pen width {_fmt(d['mean_width'])} px (thickest stroke {_fmt(d['thickest']['mean'])}), skeleton "
                      f"{_fmt(d['skeleton_length']['mean'])} px, {_fmt(d['endpoints']['mean'])} line ends, "
                      f"{_fmt(d['junction_pixels']['mean'])} junction pixels, {d['empty']} empty")
    if "shape_attributes" in metrics:
        print("\n--- Shape attributes (ink moments; coordinates in units of the image side) ---")
        for side in ("generated", "real"):
            if side in metrics["shape_attributes"]:
                print(f"{side.capitalize()}: {_shape_line(metrics['shape_attributes'][side])}")
    print("\n" + bar)


class _Args(argparse.Namespace):
    """The flags this tool adds to the reference's are opt-in all the way: they read as their default, and a command line
    without them parses to the reference's attributes and nothing else."""
    verifier_checkpoint = None
    verifier_neighbors = None
    verifier_kid = None
    components = None
    ssim = False
    strokes = False
    shape = False
    dtw = None
    modes = None


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="Evaluate trained Vanilla GAN for signature generation (MI355X HIP engine)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--checkpoint", type=str, required=True, help="Path to model checkpoint (.pt file)")
    p.add_argument("--n_samples", type=int, default=500, help="Number of samples to generate for evaluation")
    p.add_argument("--real_dir", type=str, default=None, help="Directory of real signature images to compare with")
    p.add_argument("--output_dir", type=str, default="figures/evaluation", help="Directory for grids and reports")
    p.add_argument("--batch_size", type=int, default=64, help="Batch size for sample generation")
    p.add_argument("--n_grids", type=int, default=3, help="Number of sample grids to generate")
    p.add_argument("--grid_size", type=int, default=64, help="Number of samples per grid")
    p.add_argument("--device", type=str, default=None, help="Device to use. Auto-detected if not specified.")
    p.add_argument("--seed", type=int, default=None, help="Random seed for reproducibility")
    p.add_argument("--verifier_checkpoint", type=str, default=None,
                   help="Siamese verifier checkpoint: adds a Frechet distance over its embeddings (needs --real_dir)")
    p.add_argument("--verifier_neighbors", type=int, default=None, metavar="K",
                   help="With --verifier_checkpoint and --real_dir: adds precision / recall, density / coverage and "
                        "nearest-real distances over the verifier's embeddings, from K nearest neighbours")
    p.add_argument("--verifier_kid", nargs="?", type=int, const=1000, default=argparse.SUPPRESS, metavar="PERMUTATIONS",
                   help="With --verifier_checkpoint and --real_dir: adds the Kernel Inception Distance (mean and standard deviation "
                        "over 100 subsets) and a permutation test of the RBF-kernel MMD with PERMUTATIONS label permutations over "
                        "the verifier's embeddings")
    p.add_argument("--components", nargs="?", type=lambda v: v if v == "auto" else int(v), const="auto", default=None, metavar="MIN_AREA",
                   help="Label the ink components of every generated (and real) image on the device and add a 'fragmentation' "
                        "block to the report; a component of fewer than MIN_AREA pixels counts as a speck "
                        "(MIN_AREA omitted: max(2, round(0.001 * H * W)))")
    p.add_argument("--ssim", action="store_true", default=argparse.SUPPRESS,
                   help="Add a 'pixel_similarity' block to the report: mean pairwise SSIM of the generated set (and of the real set) as "
                        "a diversity measure, and every generated image's highest SSIM to a real one against the real set's own "
                        "leave-one-out values; computed on the device, needs no network weights")
    p.add_argument("--strokes", action="store_true", default=argparse.SUPPRESS,
                   help="Add a 'stroke_geometry' block to the report: skeleton length, line ends, junction pixels and a histogram of "
                        "local pen widths of every generated (and real) image, from a thinning and an exact distance map computed on "
                        "the device; needs no network weights")
    p.add_argument("--shape", action="store_true", default=argparse.SUPPRESS,
                   help="Add a 'shape_attributes' block to the report: mass, centre, second moments, slant and spread of every "
                        "generated (and real) image's ink -- mean, standard deviation and 5 / 50 / 95th percentiles --, from exact "
                        "integer sums computed on the device; needs no network weights")
    p.add_argument("--dtw", nargs="?", type=lambda v: v if v == "auto" else int(v), const="auto", default=argparse.SUPPRESS, metavar="BAND",
                   help="Add an 'elastic_similarity' block to the report: banded dynamic time warping between the column profiles "
                        "(ink count, first and last ink row, vertical runs) of the images -- mean pairwise distance of the generated "
                        "set (and of the real set) as a diversity measure, and every generated image's lowest distance to a real one "
                        "against the real set's own leave-one-out values; tolerates shifts of up to BAND columns (BAND omitted: "
                        "max(1, width // 8)); computed on the device, needs no network weights")
    p.add_argument("--modes", nargs="?", type=lambda v: v if v == "auto" else int(v), const="auto", default=argparse.SUPPRESS, metavar="K",
                   help="With --real_dir: add a 'mode_coverage' block to the report: k-means bins of half the real set, computed on "
                        "the device, the number of statistically different bins (NDB) and the Jensen-Shannon divergence between the "
                        "real and the generated bin histograms, the real set's own hold-out floor, and the bins the Generator "
                        "produces too rarely or not at all.  Over the verifier's embeddings with --verifier_checkpoint, else over "
                        "4 x 4 box means of the pixels, which needs no network weights (K omitted: about 20 real images per bin, "
                        "between 2 and 100)")
    a = p.parse_args(argv, namespace=_Args())
    if a.modes is not None and a.modes != "auto" and not 2 <= a.modes <= 256:
        p.error("--modes K must be in [2, 256]")
    if a.modes is not None and not a.real_dir:
        p.error("--modes needs --real_dir")
    if a.dtw is not None and a.dtw != "auto" and a.dtw < 0:
        p.error("--dtw BAND must be >= 0")
    if a.verifier_kid is not None and a.verifier_kid < 1:
        p.error("--verifier_kid PERMUTATIONS must be >= 1")
    if a.components is not None and a.components != "auto" and a.components < 1:
        p.error("--components MIN_AREA must be >= 1")
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    if a.seed is not None:
        torch.manual_seed(a.seed)
        np.random.seed(a.seed)
        print(f"Random seed set to: {a.seed}")
    device = torch.device(a.device) if a.device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    print(f"Using device: {device}")
    checkpoint_path, output_dir = Path(a.checkpoint), Path(a.output_dir)
    real_dir = Path(a.real_dir) if a.real_dir else None
    try:
        generator, config = load_generator_from_checkpoint(checkpoint_path, device)
        verifier = (VerifierFeatures(Path(a.verifier_checkpoint), device, generator.output_size, a.verifier_neighbors,
                                     keep_embeddings=a.verifier_kid is not None or a.modes is not None)
                    if a.verifier_checkpoint else None)
        frag_fake = frag_real = None
        if a.components is not None:
            min_area = None if a.components == "auto" else a.components
            frag_fake, frag_real = ComponentSink(min_area), ComponentSink(min_area)
        ssim_fake, ssim_real = ((SsimSink(), SsimSink()) if a.ssim or a.dtw is not None or (a.modes is not None and verifier is None)
                                else (None, None))
        stroke_fake, stroke_real = (StrokeSink(), StrokeSink()) if a.strokes else (None, None)
        shape_fake, shape_real = (ShapeSink(), ShapeSink()) if a.shape else (None, None)
        fake = generate_samples(generator, a.n_samples, generator.latent_dim, device, a.batch_size,
                                keep_images=max(0, a.n_grids) * a.grid_size,
                                embedding_sink=verifier.sink() if verifier is not None else None, component_sink=frag_fake,
                                ssim_sink=ssim_fake, stroke_sink=stroke_fake, shape_sink=shape_fake)
        print("\nCreating sample grids...")
        grid_paths = create_sample_grids(fake, output_dir, a.n_grids, a.grid_size)
        real = verifier_real = None
        if real_dir:
            try:
                if verifier is not None and verifier.input_resize is not None:
                    real, verifier_real = load_real_images(real_dir, a.n_samples, generator.output_size, device, VERIFIER_IMAGE_SIZE,
                                                           component_sink=frag_real, ssim_sink=ssim_real,
                                                           stroke_sink=stroke_real, shape_sink=shape_real)
                else:
                    real = load_real_images(real_dir, a.n_samples, generator.output_size, device, component_sink=frag_real,
                                            ssim_sink=ssim_real, stroke_sink=stroke_real, shape_sink=shape_real)
            except Exception as e:                              # noqa: BLE001 -- the evaluation goes on without them
                print(f"Warning: Could not load real images: {e}")
        print("\nComputing evaluation metrics...")
        metrics = compute_metrics(fake, real, device, verifier, a.verifier_neighbors, verifier_real,
                                  fragmentation_block(frag_fake, frag_real) if frag_fake is not None else None,
                                  pixel_similarity_block(ssim_fake, ssim_real) if a.ssim else None,
                                  stroke_geometry_block(stroke_fake, stroke_real) if a.strokes else None,
                                  shape_attributes_block(shape_fake, shape_real) if a.shape else None,
                                  kid_permutations=a.verifier_kid,
                                  elastic_similarity=(elastic_similarity_block(ssim_fake, ssim_real, None if a.dtw == "auto" else a.dtw)
                                                      if a.dtw is not None else None),
                                  modes=(dict(k=None if a.modes == "auto" else a.modes, generated=ssim_fake, real=ssim_real)
                                         if a.modes is not None else None))
        report_path = save_evaluation_report(metrics, config, output_dir, checkpoint_path, grid_paths)
        print_summary(metrics)
        print("\nEvaluation complete!")
        print(f"  Sample grids saved to: {output_dir}")
        print(f"  Report saved to: {report_path}")
        return 0
    except FileNotFoundError as e:
        print(f"Error: {e}")
        return 1
    except Exception as e:                                      # noqa: BLE001
        print(f"Evaluation failed: {e}")
        import traceback
        traceback.print_exc()
        return 1


if __name__ == "__main__":
    sys.exit(main())
