"""Drop-in for the reference's ``utils/inference.py`` (checkpoint -> Generator, batched generation,
tensor -> PIL) on the MI355X HIP engine.

Checkpoint tolerance is the reference's (utils/inference.py:20-104): a dict with
``generator_state_dict`` (trainer layout A / VanillaGAN layout B), a dict with ``state_dict``, or a
bare Generator state_dict whose architecture is inferred from ``fc.*weight.shape[1]`` and the count
of ``upsample_blocks.N.block.0.weight`` keys (>= 5 -> 128x128).

Realism-filtered generation (the reference app's "Filter by Realism", app_vanilla_gan_signatures.py:1065-1385, which is not UI:
it is where a trained Discriminator is used after training) lives here too: ``load_discriminator``, ``binarize_uint8`` /
``process_images``, ``filter_plan`` and ``generate_signatures_filtered``.

So does the way back from an image to a latent vector: ``project_signatures`` (an Adam loop on z around
Engine.g_latent_objective_grad), and on top of it the app's second generation tab, "Morphing" (app_vanilla_gan_signatures.py:1631-1717):
``morph_blend``, ``morph_sequence`` and ``morph_strip``.

Realism-guided refinement joins the two: ``refine_latents`` moves latent vectors up the Discriminator's eval-mode score (an
Adam loop on z around Engine.g_latent_objective_grad) instead of throwing low-scoring images away,
``generate_signatures_refined`` is generation on top of it, and ``project_signatures`` takes the same realism and prior terms
beside its pixel error.  ``adopt_discriminator`` brings the Discriminator into the Generator's context for them.

``generate_signatures_diverse`` takes the filter's pool and selects from it for diversity in the verifier's embedding space
(utils/diverse.py) instead of keeping the top of the ranking.

``edit_latents`` changes a generated signature's shape attributes -- slant, size, boldness, position: the ink moments of
shape.py -- while it stays the same signature: an Adam loop on z around shape.shape_grad, whose image-space gradient the seeded
Engine.g_latent_objective_grad carries to z; ``generate_signatures_edited`` is generation on top of it."""
import math
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..discriminator_vanilla_gan import Discriminator
from ..generator_vanilla_gan import Generator

DEFAULT_LATENT_DIM, DEFAULT_IMAGE_SIZE, DEFAULT_IMAGE_CHANNELS = 100, 64, 1


def infer_architecture_from_state_dict(state_dict: Dict[str, Any]) -> Tuple[int, int]:
    latent_dim, blocks = DEFAULT_LATENT_DIM, 0
    for key, t in state_dict.items():
        if "fc" in key and "weight" in key and getattr(t, "dim", lambda: 0)() == 2:
            latent_dim = int(t.shape[1])
            break
    for key in state_dict:
        if "upsample_blocks" in key and ".0.weight" in key:
            try:
                blocks = max(blocks, int(key.split(".")[1]) + 1)
            except ValueError:
                pass
    return latent_dim, (128 if blocks >= 5 else 64)


def load_generator(checkpoint_path: str, device: torch.device) -> Tuple[Generator, int]:
    """(Generator in eval mode on ``device``, latent_dim).  Only the safe loader is used."""
    g, latent_dim, _ = load_generator_and_config(checkpoint_path, device)
    return g, latent_dim


def load_generator_and_config(checkpoint_path: str, device: torch.device) -> Tuple[Generator, int, Dict[str, Any]]:
    """load_generator plus the checkpoint's ``config`` dict ({} where the file has none): what the evaluation report records."""
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    channels = DEFAULT_IMAGE_CHANNELS
    cfg: Dict[str, Any] = {}
    if isinstance(ck, dict) and ("generator_state_dict" in ck or "state_dict" in ck):
        cfg = ck.get("config", {}) or {}
        latent_dim = cfg.get("latent_dim", DEFAULT_LATENT_DIM)
        size = cfg.get("image_size", DEFAULT_IMAGE_SIZE)
        channels = cfg.get("image_channels", DEFAULT_IMAGE_CHANNELS)
        sd = ck["generator_state_dict"] if "generator_state_dict" in ck else ck["state_dict"]
    else:
        sd = ck
        latent_dim, size = infer_architecture_from_state_dict(sd)
    g = Generator(latent_dim=latent_dim, output_size=size, output_channels=channels)
    g.load_state_dict(sd)
    g.to(device)
    g.eval()
    return g, latent_dim, dict(cfg)


def tensor_to_uint8(images: torch.Tensor) -> np.ndarray:
    """(B,1,H,W) in [-1,1] -> (B,H,W) uint8 with the reference's rule ((x+1)*127.5, clip, TRUNCATE)."""
    x = images.detach().float().cpu().numpy()
    return ((x[:, 0] + 1) * 127.5).clip(0, 255).astype(np.uint8)


_pinned: Dict[Any, torch.Tensor] = {}       # one reused page-locked staging buffer per device (grown, never shrunk)


def _to_host_u8(u8: torch.Tensor) -> np.ndarray:
    """Device uint8 tensor -> numpy array of the same shape: one byte per pixel through the pinned buffer."""
    n = u8.numel()
    buf = _pinned.get(u8.device)
    if buf is None or buf.numel() < n:
        buf = _pinned[u8.device] = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True)
    buf[:n].copy_(u8.reshape(-1), non_blocking=True)
    torch.cuda.current_stream(u8.device).synchronize()
    return buf[:n].numpy().reshape(tuple(u8.shape)).copy()       # (the buffer is reused by the next call)


class Despeckle:
    """The settings of ``generate_signatures --despeckle`` and what the cleaning has removed so far: every ink component
    (byte < ``threshold``, ``connectivity``-connected) of fewer than ``min_area`` pixels becomes white (255), every other byte
    stays what it is (components.despeckle_u8, on the device).  ``min_area`` None: components.default_min_area of the first
    images cleaned.  ``clean_device`` / ``clean_host`` return the (N, 9) component counters of the images BEFORE cleaning;
    ``count`` adds the removed components and pixels of such rows to the totals ``report`` hands out."""

    def __init__(self, min_area: Optional[int] = None, threshold: int = 128, connectivity: int = 8) -> None:
        if not 1 <= int(threshold) <= 255:
            raise ValueError(f"despeckle needs an ink threshold in 1..255, got {threshold}")
        if min_area is not None and int(min_area) < 1:
            raise ValueError(f"min_area = {min_area} < 1")
        self.min_area, self.threshold, self.connectivity = min_area, int(threshold), int(connectivity)
        self.removed_components = self.removed_pixels = 0

    def clean_device(self, u8: torch.Tensor) -> torch.Tensor:
        """Clean the contiguous uint8 (N, H, W) device tensor IN PLACE -> int32 (N, 9) device counters of its former content."""
        from ..components import default_min_area, despeckle_u8
        if self.min_area is None:
            self.min_area = default_min_area(u8.shape[-2], u8.shape[-1])
        stats = torch.empty(u8.shape[0], 9, dtype=torch.int32, device=u8.device)
        despeckle_u8(u8, self.threshold, self.connectivity, self.min_area, 255, out=u8, stats=stats)
        return stats

    def clean_host(self, u8: np.ndarray, device: torch.device) -> Tuple[np.ndarray, np.ndarray]:
        """(N, H, W) uint8 on the host -> (cleaned copy, (N, 9) counters), through the device."""
        t = torch.from_numpy(np.ascontiguousarray(u8)).to(device)
        stats = self.clean_device(t)
        return _to_host_u8(t), stats.cpu().numpy()

    def count(self, stats) -> None:
        from ..components import SMALL_COMPONENTS, SMALL_INK
        rows = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
        rows = rows.reshape(-1, 9).astype(np.int64)
        self.removed_components += int(rows[:, SMALL_COMPONENTS].sum())
        self.removed_pixels += int(rows[:, SMALL_INK].sum())

    def report(self) -> Dict[str, int]:
        return {"min_area": self.min_area, "threshold": self.threshold, "connectivity": self.connectivity,
                "removed_components": self.removed_components, "removed_pixels": self.removed_pixels}


class PenWidth:
    """The settings of ``generate_signatures --pen_width`` and what the redraw has measured so far: every image is thinned to
    its centre line and drawn again with a disc of squared radius ``strokes.radius2_for_pen_width(width)`` -- ink (byte <
    ``threshold``) becomes 0, paper 255 (strokes.restroke_u8, on the device).  ``redraw_device`` adds the width histograms of the
    images before (from the redraw's own launch) and after (a second launch on the result) to the totals ``report`` hands
    out as mean widths."""

    def __init__(self, width: int, threshold: int = 128) -> None:
        from ..strokes import WIDTH_BINS, radius2_for_pen_width
        if not 1 <= int(threshold) <= 255:
            raise ValueError(f"pen width needs an ink threshold in 1..255, got {threshold}")
        self.width, self.radius2, self.threshold = int(width), radius2_for_pen_width(width), int(threshold)
        self.before, self.after = np.zeros(WIDTH_BINS, np.int64), np.zeros(WIDTH_BINS, np.int64)

    def redraw_device(self, u8: torch.Tensor) -> None:
        """Redraw the contiguous uint8 (N, H, W) device tensor IN PLACE."""
        from ..strokes import COUNT, WIDTH_HIST, restroke_u8, stroke_stats
        stats = torch.empty(u8.shape[0], COUNT, dtype=torch.int32, device=u8.device)
        restroke_u8(u8, self.radius2, self.threshold, 0, 255, out=u8, stats=stats)
        after = stroke_stats(u8, self.threshold)
        self.before += stats[:, WIDTH_HIST:].sum(dim=0, dtype=torch.int64).cpu().numpy()
        self.after += after[:, WIDTH_HIST:].sum(dim=0, dtype=torch.int64).cpu().numpy()

    def redraw_host(self, u8: np.ndarray, device: torch.device) -> np.ndarray:
        """(N, H, W) uint8 on the host -> the redrawn copy, through the device."""
        t = torch.from_numpy(np.ascontiguousarray(u8)).to(device)
        self.redraw_device(t)
        return _to_host_u8(t)

    @staticmethod
    def _mean(hist: np.ndarray) -> Optional[float]:
        widths = 2 * np.arange(1, len(hist) + 1, dtype=np.int64) - 1
        return float(int((hist * widths).sum()) / int(hist.sum())) if hist.sum() else None

    def report(self) -> Dict[str, Any]:
        return {"pen_width": self.width, "radius2": self.radius2, "threshold": self.threshold,
                "mean_width_before": self._mean(self.before), "mean_width_after": self._mean(self.after)}


def generate_uint8(generator: Generator, z: torch.Tensor, despeckle: Optional[Despeckle] = None,
                   pen_width: Optional[PenWidth] = None) -> np.ndarray:
    """z (B, latent) -> (B, H, W) uint8, the bytes of ``tensor_to_uint8(generator(z))``.  In eval mode the Generator's last
    kernel writes them itself (Engine.g_generate_u8) and one byte per pixel crosses to the host; a Generator left in train()
    mode (BatchNorm batch statistics) has no such kernel and takes the fp32 route.  ``despeckle``: the bytes are cleaned
    (and what was removed is counted) before they are returned -- on the device, before the copy, in eval mode.
    ``pen_width``: the bytes are then redrawn at that pen width, on the device as well."""
    if generator.training:
        u8 = tensor_to_uint8(generator(z))
        if despeckle is not None:
            u8, stats = despeckle.clean_host(u8, z.device)
            despeckle.count(stats)
        if pen_width is not None:
            u8 = pen_width.redraw_host(u8, z.device)
        return u8
    u8 = generator._require_engine().g_generate_u8(z)
    if despeckle is not None:
        despeckle.count(despeckle.clean_device(u8))
    if pen_width is not None:
        pen_width.redraw_device(u8)
    return _to_host_u8(u8)


def tensor_to_pil_image(tensor: torch.Tensor):
    from PIL import Image
    return Image.fromarray(tensor_to_uint8(tensor.unsqueeze(0))[0], mode="L")


def generate_signatures_batch(generator: Generator, n_samples: int, latent_dim: int, device: torch.device,
                              seed: Optional[int] = None, batch_size: int = 32, progress_callback=None,
                              noise_scale: float = 1.0, despeckle: Optional[Despeckle] = None,
                              pen_width: Optional[PenWidth] = None) -> List[Any]:
    """Reference semantics (utils/inference.py:136-194): optional torch.manual_seed, then per batch
    z = randn(b, latent, device=device) * noise_scale -> generator(z) -> one PIL image per sample.  ``despeckle``: every
    batch's bytes are cleaned on the way (generate_uint8); ``pen_width``: and then redrawn at that pen width."""
    extra = {} if pen_width is None else {"pen_width": pen_width}
    from PIL import Image
    if seed is not None:
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)
    out: List[Any] = []
    done = 0
    while done < n_samples:
        b = min(batch_size, n_samples - done)
        z = torch.randn(b, latent_dim, device=device) * noise_scale
        for arr in generate_uint8(generator, z, despeckle, **extra):
            out.append(Image.fromarray(arr, mode="L"))
        done += b
        if progress_callback is not None:
            progress_callback(done / n_samples)
    return out


# ---- realism-filtered generation -------------------------------------------------------------------------------------
def load_discriminator(checkpoint_path: str, device: torch.device, image_size: int = 64) -> Optional[Discriminator]:
    """The checkpoint's Discriminator in eval mode on ``device`` (app_vanilla_gan_signatures.py:580-614); ``None`` where
    the file is not a dict or holds no ``discriminator_state_dict``.  Only the safe loader is used.  Two deliberate
    differences from the reference: a state dict with ``weight_orig`` keys (a run trained with use_spectral_norm=True) builds
    ``Discriminator(use_spectral_norm=True)`` -- the reference builds the plain network, fails in load_state_dict and swallows
    that into ``None`` -- and every error other than the missing key propagates instead of becoming ``None``."""
    ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)
    if not isinstance(ck, dict) or "discriminator_state_dict" not in ck:
        return None
    sd = ck["discriminator_state_dict"]
    d = Discriminator(input_size=image_size, use_spectral_norm=any(k.endswith("weight_orig") for k in sd))
    d.load_state_dict(sd)
    d.to(device)
    d.eval()
    return d


def binarize_uint8(u8: np.ndarray, threshold: int) -> np.ndarray:
    """byte < threshold ? 0 : 255 -- the bytes of process_images' ``img.point(fn, mode='1')`` seen as grayscale again."""
    return np.where(np.asarray(u8) < int(threshold), 0, 255).astype(np.uint8)


def process_images(images: List[Any], threshold: int = 127, make_transparent: bool = False) -> List[Any]:
    """app_vanilla_gan_signatures.py:863-904: every image becomes a mode '1' image (pixels < threshold black, the rest
    white), or with ``make_transparent`` an RGBA image whose white pixels are (255, 255, 255, 0) and whose ink is
    (0, 0, 0, 255)."""
    from PIL import Image
    out = []
    for img in images:
        binary = binarize_uint8(np.array(img.convert("L")), threshold)
        if make_transparent:
            ink = binary == 0
            rgba = np.empty(binary.shape + (4,), dtype=np.uint8)
            rgba[..., :3] = np.where(ink, 0, 255)[..., None]
            rgba[..., 3] = np.where(ink, 255, 0)
            out.append(Image.fromarray(rgba))
        else:
            out.append(Image.fromarray(binary, mode="L").convert("1"))       # {0, 255} only: no dithering takes place
    return out


def filter_plan(n_signatures: int, oversampling_ratio: float, batch_size: int, seed: Optional[int]
                ) -> Tuple[int, List[Tuple[int, Optional[int]]]]:
    """(total, [(batch size, batch seed), ...]) of a filtered generation (app_vanilla_gan_signatures.py:1280,1333-1338):
    total = int(n * ratio) images in batches of ``batch_size`` (a ragged last one), batch number i seeded ``seed + i``, or
    not at all without a seed.  Pure host code."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    total = int(n_signatures * oversampling_ratio)
    plan, done = [], 0
    while done < total:
        b = min(batch_size, total - done)
        plan.append((b, seed + done // batch_size if seed is not None else None))
        done += b
    return total, plan


def _seed_batch(seed: Optional[int]) -> None:
    """What generate_signatures_batch(seed=seed) does before it draws."""
    if seed is not None:
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)


def dequantize_uint8(u8: np.ndarray) -> torch.Tensor:
    """(B, H, W) uint8 -> (B, 1, H, W) fp32 on the CPU by the reference's expression (app_vanilla_gan_signatures.py:1368):
    a true fp32 division, then a subtraction."""
    return (torch.from_numpy(np.ascontiguousarray(u8)).float() / 127.5 - 1.0).unsqueeze(1)


def _scored_pool(g_eng, d_eng, total, plan, latent_dim, device, noise_scale, binarize, despeckle=None, tick=None):
    """The device route's pool: (pool uint8 (total, S, S), scores fp32 (total,), removed int32 (total, 9) or None), all on the
    Generator's device.  Batch by batch (``plan``: filter_plan's), seeded, z = randn * noise_scale, the Generator's last kernel
    writes the bytes into the pool, ``despeckle`` cleans them IN PLACE (``removed``: the counters of what they were) and the
    Discriminator scores them where they lie, binarised on load when ``binarize`` is a byte value.  ``tick(b)`` after every batch.
    generate_signatures_filtered and generate_signatures_diverse both build their pool here, so for equal arguments the two
    hold the same bytes and scores."""
    size = g_eng.image_size
    pool = torch.empty(total, size, size, dtype=torch.uint8, device=g_eng.device)
    scores = torch.empty(total, dtype=torch.float32, device=g_eng.device)
    removed = torch.empty(total, 9, dtype=torch.int32, device=g_eng.device) if despeckle is not None else None
    done = 0
    for b, batch_seed in plan:
        _seed_batch(batch_seed)
        z = torch.randn(b, latent_dim, device=device) * noise_scale
        g_eng.g_generate_u8(z, out=pool[done:done + b])
        if despeckle is not None:
            removed[done:done + b] = despeckle.clean_device(pool[done:done + b])
        d_eng.d_score_u8(pool[done:done + b], binarize=binarize, out=scores[done:done + b])
        done += b
        if tick is not None:
            tick(b)
    return pool, scores, removed


def generate_signatures_filtered(generator: Generator, discriminator: Discriminator, n_signatures: int, latent_dim: int,
                                 device: torch.device, seed: Optional[int] = None, batch_size: int = 32,
                                 oversampling_ratio: float = 2.0, noise_scale: float = 1.0, threshold: Optional[int] = None,
                                 route: str = "device", progress_callback=None, despeckle: Optional[Despeckle] = None
                                 ) -> Tuple[List[Any], List[float]]:
    """The reference app's "Filter by Realism": generate int(n * ratio) signatures batch by batch (filter_plan), binarise them
    when ``threshold`` is given, score each with the Discriminator on byte / 127.5 - 1.0, and return the best min(n, total)
    as (PIL 'L' images, scores), highest score first, equal scores in generation order.

    route="device": the bytes go from the Generator's last kernel into a pool in HBM, the Discriminator's first block reads
    them there (Engine.d_score_u8) and writes into the pool's score vector; after the last batch one select_topk and one
    gather_u8 run, and only the selected images and scores cross to the host.  route="host": the reference's loop on the
    existing pieces -- bytes to the host, numpy binarisation, CPU dequantisation, Discriminator.forward, Python's sort.  Both
    give identical images and scores.  The device route falls back to the host route where it does not apply: a Generator or
    Discriminator in train() mode, or more than _lib.SELECT_MAX images.

    ``despeckle``: every batch is cleaned IN PLACE in the pool before it is scored (and before ``threshold`` binarises it on
    load), so a returned score belongs to the image that is returned; what was removed from the RETURNED images is counted."""
    from PIL import Image
    from .. import _lib
    if route not in ("device", "host"):
        raise ValueError(f"route must be 'device' or 'host', got {route!r}")
    if threshold is not None and not 0 <= int(threshold) <= 255:
        raise ValueError(f"threshold must be a byte value, got {threshold}")
    total, plan = filter_plan(n_signatures, oversampling_ratio, batch_size, seed)
    keep = min(int(n_signatures), total)
    if keep < 1:
        return [], []
    if generator.training or discriminator.training or total > _lib.SELECT_MAX:
        route = "host"
    done = 0

    def tick(b):
        nonlocal done
        done += b
        if progress_callback is not None:
            progress_callback(done / total)

    if route == "host":
        records = []
        for b, batch_seed in plan:
            _seed_batch(batch_seed)
            z = torch.randn(b, latent_dim, device=device) * noise_scale
            u8 = generate_uint8(generator, z)
            removed = np.zeros((b, 9), np.int32)
            if despeckle is not None:
                u8, removed = despeckle.clean_host(u8, device)
            if threshold is not None:
                u8 = binarize_uint8(u8, threshold)
            with torch.no_grad():
                scores = discriminator(dequantize_uint8(u8).to(device)).cpu().numpy().flatten().tolist()
            records += [(arr, float(sc), row) for arr, sc, row in zip(u8, scores, removed)]
            tick(b)
        records.sort(key=lambda r: r[1], reverse=True)
        records = records[:keep]
        if despeckle is not None:
            despeckle.count(np.stack([row for _, _, row in records]))
        records = [(arr, sc) for arr, sc, _ in records]
        return [Image.fromarray(arr, mode="L") for arr, _ in records], [sc for _, sc in records]

    g_eng = generator._require_engine()
    binarize = None if threshold is None else int(threshold)
    pool, scores, removed = _scored_pool(g_eng, discriminator._require_engine(), total, plan, latent_dim, device, noise_scale,
                                         binarize, despeckle, tick)
    index = g_eng.select_topk(scores, keep)
    if despeckle is not None:
        despeckle.count(removed[index.long()])
    picked = _to_host_u8(g_eng.gather_u8(pool, index, binarize=binarize))
    best = _to_host_u8(scores[index.long()].view(torch.uint8)).view(np.float32)
    return [Image.fromarray(arr, mode="L") for arr in picked], [float(sc) for sc in best]


# ---- diversity-aware selection from the filter's pool ----------------------------------------------------------------------
def _as_u8_images(name: str, images, size: int, device: torch.device) -> torch.Tensor:
    t = torch.as_tensor(np.ascontiguousarray(images) if isinstance(images, np.ndarray) else images)
    if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape[1:]) != (size, size) or t.shape[0] < 1:
        raise ValueError(f"{name} must be uint8 (N >= 1, {size}, {size}), got {t.dtype} {tuple(t.shape)}")
    return t.to(device).contiguous()


def _embed_u8(verifier, u8: torch.Tensor, resize: bool) -> torch.Tensor:
    """The verifier's embeddings of uint8 (N, S, S) device images, max_images at a time: embed_u8, or embed_resized."""
    embed = verifier.embed_resized if resize else verifier.embed_u8
    step = int(verifier.max_images)
    return torch.cat([embed(u8[i:i + step]) for i in range(0, u8.shape[0], step)]).contiguous()


def _nn_d2(emb: torch.Tensor) -> Optional[np.ndarray]:
    """Every row's squared distance to its nearest other row, on the host; None for fewer than two rows."""
    from .neighbors import knn
    if emb.shape[0] < 2:
        return None
    return knn(emb, emb, 1, exclude_self=True)[0][:, 0].cpu().numpy()


def generate_signatures_diverse(generator: Generator, discriminator: Discriminator, verifier, n_signatures: int, latent_dim: int,
                                device: torch.device, seed: Optional[int] = None, batch_size: int = 32,
                                oversampling_ratio: float = 4.0, keep_ratio: float = 0.5, noise_scale: float = 1.0,
                                threshold: Optional[int] = None, real_u8=None, memorisation_ratio: Optional[float] = None,
                                existing_u8=None, min_separation: float = 0.0, despeckle: Optional[Despeckle] = None,
                                verifier_resize: bool = False, return_pool: bool = False) -> Tuple[List[Any], List[float], Dict[str, Any]]:
    """Diversity-aware selection from the realism filter's pool: generate int(n * ratio) signatures exactly as the device route
    of generate_signatures_filtered does (the same filter_plan, batch seeds, in-place despeckle and d_score_u8, so pool bytes
    and scores are the filter's bit for bit), embed the bytes that will be written (the binarised pool with ``threshold``)
    with the Siamese ``verifier`` (embed_u8; ``verifier_resize``: embed_resized, for a 128x128 Generator), and pick up to
    min(n, total) signatures that are mutually farthest apart in that space (utils.diverse.select_diverse), among the
    eligible ones: the ceil(keep_ratio * total) most realistic (utils.diverse.eligibility).

    ``real_u8`` (N, S, S) uint8 with ``memorisation_ratio`` (they come together; the ratio has no default): a candidate whose
    nearest real embedding is closer than memorisation_ratio * the median of the real set's own leave-one-out nearest
    distances is not eligible.  ``existing_u8``: a synthetic set grown in earlier runs; the picks keep away from it as they
    do from each other (its nearest-member distances are the selection's anchors).  ``min_separation``: stop once the best
    remaining candidate is closer than this to what is kept, so fewer than n may come back.  Without anchors the first pick is
    the eligible signature with the highest realism score; with anchors it is the one farthest from them.

    Returns (PIL 'L' images in pick order, their scores, report): utils.diverse.diversity_summary's dictionary -- what was
    picked and why the run ended, each pick's gain, and the nearest-neighbour distances and mean realism inside this
    selection beside those of the plain top-n-by-realism selection of the same pool: what was bought and what it cost.
    ``return_pool``: report['_device'] holds the device tensors {pool, scores, embeddings, eligible}.  Of the pool only the
    selected images, their scores and the pick lists cross to the host, beside the numbers the report is made of (the
    nearest-neighbour and nearest-real distances of the two selections of n, one coverage figure).  The host waits for the
    device three times on the way: for the number of eligible rows and the first pick (two scalars) before the selection is
    enqueued, for the number of picks after it, and for the selected bytes.

    There is no host route: a Generator, Discriminator or verifier in train() mode, or a pool larger than _lib.SELECT_MAX,
    raises ValueError."""
    from PIL import Image
    from .. import _lib
    from .diverse import diversity_summary, eligibility, select_diverse
    from .neighbors import knn
    if threshold is not None and not 0 <= int(threshold) <= 255:
        raise ValueError(f"threshold must be a byte value, got {threshold}")
    if (real_u8 is None) != (memorisation_ratio is None):
        raise ValueError("real_u8 and memorisation_ratio come together: the memorisation floor is memorisation_ratio times the "
                         "real set's median leave-one-out nearest distance, and the ratio has no default")
    if memorisation_ratio is not None and not float(memorisation_ratio) >= 0.0:
        raise ValueError(f"memorisation_ratio must be >= 0, got {memorisation_ratio}")
    if not float(min_separation) >= 0.0:
        raise ValueError(f"min_separation must be >= 0, got {min_separation}")
    if not 0.0 < float(keep_ratio) <= 1.0:
        raise ValueError(f"keep_ratio must be in (0, 1], got {keep_ratio}")
    if generator.training or discriminator.training or verifier.training:
        raise ValueError("diverse selection has no host route: call .eval() on the Generator, the Discriminator and the verifier")
    if generator.output_size != 64 and not verifier_resize:
        raise ValueError(f"the verifier reads 64x64 images: a {generator.output_size}x{generator.output_size} Generator needs "
                         "verifier_resize=True")
    total, plan = filter_plan(n_signatures, oversampling_ratio, batch_size, seed)
    if total > _lib.SELECT_MAX:
        raise ValueError(f"diverse selection has no host route: a pool of {total} signatures exceeds {_lib.SELECT_MAX}")
    keep = min(int(n_signatures), total)
    if keep < 1:
        return [], [], diversity_summary(max(total, 0), 0, max(keep, 0), [], [], 0, [])
    g_eng = generator._require_engine()
    dev, size = g_eng.device, g_eng.image_size
    real = existing = None
    if real_u8 is not None:
        real = _as_u8_images("real_u8", real_u8, size, dev)
        if real.shape[0] < 2:
            raise ValueError("the memorisation floor needs at least two real signatures")
    if existing_u8 is not None:
        existing = _as_u8_images("existing_u8", existing_u8, size, dev)
    binarize = None if threshold is None else int(threshold)
    pool, scores, removed = _scored_pool(g_eng, discriminator._require_engine(), total, plan, latent_dim, device, noise_scale,
                                         binarize, despeckle)
    everything = torch.arange(total, dtype=torch.int32, device=dev)
    written = pool if binarize is None else g_eng.gather_u8(pool, everything, binarize=binarize)
    emb = _embed_u8(verifier, written, verifier_resize)

    near_d2 = floor2 = None
    if real is not None:
        real_emb = _embed_u8(verifier, real, verifier_resize)
        near_d2 = knn(emb, real_emb, 1)[0][:, 0].contiguous()
        loo = knn(real_emb, real_emb, 1, exclude_self=True)[0][:, 0].sqrt().sort().values
        median = 0.5 * (loo[(loo.numel() - 1) // 2] + loo[loo.numel() // 2])                 # numpy's median, on the device
        floor2 = (float(memorisation_ratio) * median) ** 2
    mask = eligibility(scores, keep_ratio, near_d2, floor2)
    anchor_d2 = None
    if existing is not None:
        existing_emb = _embed_u8(verifier, existing, verifier_resize)
        anchor_d2 = knn(emb, existing_emb, 1)[0][:, 0].contiguous()
    rank = g_eng.select_topk(scores, total)                                                 # the filter's order of the pool
    eligible_in_rank = torch.nonzero(mask[rank.long()]).flatten()
    n_eligible = int(eligible_in_rank.numel())
    first = int(rank[eligible_in_rank[0]]) if anchor_d2 is None and n_eligible else None

    order, gain2, count, min_d2 = select_diverse(emb, keep, mask, anchor_d2, first, min_separation)
    count_h = int(count.cpu()[0])
    picks = order[:count_h].contiguous()
    top = rank[:keep].contiguous()
    coverage = float(min_d2[mask.bool()].max().cpu()) if n_eligible else None
    report = diversity_summary(total, n_eligible, keep, order.cpu().numpy(), gain2.cpu().numpy(), count_h,
                               scores[picks.long()].cpu().numpy(),
                               None if near_d2 is None else near_d2[picks.long()].cpu().numpy(), coverage,
                               _nn_d2(emb[picks.long()].contiguous()), scores[top.long()].cpu().numpy(),
                               _nn_d2(emb[top.long()].contiguous()))
    if return_pool:
        report["_device"] = {"pool": pool, "scores": scores, "embeddings": emb, "eligible": mask}
    if count_h == 0:
        return [], [], report
    if despeckle is not None:
        despeckle.count(removed[picks.long()])
    picked = _to_host_u8(g_eng.gather_u8(pool, picks, binarize=binarize))
    best = _to_host_u8(scores[picks.long()].view(torch.uint8)).view(np.float32)
    return [Image.fromarray(arr, mode="L") for arr in picked], [float(sc) for sc in best], report


# ---- projection into the latent space and morphing ---------------------------------------------------------------------
def load_target_images(path: str, image_size: int) -> Tuple[List[str], np.ndarray]:
    """(file names, (N, S, S) uint8): the image file ``path``, or the images of the directory ``path`` in the loader's sorted
    order, decoded and resized as evaluate_vanilla_gan_signatures.load_real_images does it (SignatureDataset.decode: PIL ->
    'L' -> bilinear resize).  An unreadable file raises."""
    import os
    from pathlib import Path
    from ..data_loader_signatures import SignatureDataset
    p = Path(path)
    if not p.exists():
        raise FileNotFoundError(f"no such image file or directory: {path}")
    ds = SignatureDataset(p if p.is_dir() else p.parent)
    if not p.is_dir():
        ds.image_paths = [p]
    if len(ds) == 0:
        raise ValueError(f"No images found in {path}")
    names, out = [], []
    for i in range(len(ds)):
        arr = ds.decode(i, image_size)
        if arr is None:
            raise ValueError(f"unreadable image: {ds.get_image_path(i)}")
        names.append(os.path.basename(str(ds.get_image_path(i)))); out.append(arr)
    return names, np.stack(out)


def projection_plan(n_targets: int, restarts: int, max_batch: int) -> List[Tuple[int, int, int]]:
    """[(restart, first target, count), ...]: the batches of a projection, in the order they run.  Every restart walks the
    targets in the same chunks of ``max_batch``, so the batch a candidate is optimised in -- and with it the kernels the
    library picks, whose summation orders follow the batch size -- does not depend on how many restarts were asked for:
    restart r of a run with R restarts is bit for bit the run with one restart seeded ``seed + r``.  Pure host code."""
    if n_targets < 0 or restarts < 1 or max_batch < 1:
        raise ValueError(f"need n_targets >= 0, restarts >= 1, max_batch >= 1, got {n_targets}, {restarts}, {max_batch}")
    return [(r, t0, min(max_batch, n_targets - t0)) for r in range(restarts) for t0 in range(0, n_targets, max_batch)]


def projection_starts(n_targets: int, latent_dim: int, restart: int, z0: Optional[torch.Tensor] = None,
                      seed: Optional[int] = None) -> torch.Tensor:
    """(n_targets, latent) fp32 on the CPU: where restart number ``restart`` starts.  Restart 0 starts at ``z0`` when that is
    given; every other start is N(0, 1) from a CPU generator seeded ``seed + restart`` (unseeded: torch's global generator)."""
    if restart == 0 and z0 is not None:
        z0 = torch.as_tensor(z0, dtype=torch.float32).cpu()
        if tuple(z0.shape) != (n_targets, latent_dim):
            raise ValueError(f"z0 must be ({n_targets}, {latent_dim}), got {tuple(z0.shape)}")
        return z0.clone()
    gen = None if seed is None else torch.Generator().manual_seed(int(seed) + restart)
    return torch.randn(n_targets, latent_dim, generator=gen)


def discriminator_adoption(generator: Generator, discriminator: Discriminator) -> str:
    """How ``discriminator`` comes into the Generator's context: 'shared' -- both modules already run on one engine, nothing is
    copied -- or 'copy' -- the Generator's engine is its own and the Discriminator is the plain (no spectral norm) module of
    the same image size: its parameters are copied into that engine's Discriminator arena.  Anything else raises ValueError.
    Both modules must be in eval() mode.  Pure host code (it reads module attributes only)."""
    if generator.training or discriminator.training:
        raise ValueError("the latent objective runs both networks in eval mode: call .eval() on the Generator and the Discriminator")
    if generator._engine is not None and generator._engine is discriminator._engine:
        return "shared"
    if not generator._shared_engine and not discriminator.use_spectral_norm and discriminator.input_size == generator.output_size:
        return "copy"
    raise ValueError("the Discriminator cannot be copied into the Generator's context (a spectral-norm Discriminator, another "
                     "image size, or a Generator on a shared engine): build both modules on one engine -- pass it as the "
                     "`_engine` constructor argument of Generator and Discriminator, as VanillaGAN does")


def adopt_discriminator(generator: Generator, discriminator: Discriminator):
    """The engine that holds both networks (discriminator_adoption): the shared one, or the Generator's own after the
    Discriminator's parameters were copied into its views('d') and params_changed() was called.  Call once per public call."""
    how = discriminator_adoption(generator, discriminator)
    eng = generator._require_engine()
    if how == "copy":
        if eng.spectral_norm or abs(eng.leaky_slope - discriminator.leaky_slope) > 1e-12:
            raise ValueError("the Generator's engine was created with another spectral_norm / leaky_slope setting than the "
                             "Discriminator: build both modules on one engine (the `_engine` constructor argument)")
        views = eng.views("d")
        with torch.no_grad():
            for name, p in discriminator.named_parameters():
                views[name].copy_(p.detach().to(eng.device))
        eng.params_changed()
    return eng


def refine_plan(n: int, max_batch: int) -> List[Tuple[int, int]]:
    """[(first vector, count), ...]: the chunks of ``max_batch`` a refinement of ``n`` latent vectors runs in.  Pure host code."""
    if n < 0 or max_batch < 1:
        raise ValueError(f"need n >= 0 and max_batch >= 1, got {n}, {max_batch}")
    return [(t0, min(max_batch, n - t0)) for t0 in range(0, n, max_batch)]


def _check_refine(steps, lr, realism_weight, prior_weight):
    from ..engine import check_objective_weights
    if steps < 1 or not lr > 0:
        raise ValueError(f"steps must be >= 1 and lr > 0, got {steps}, {lr}")
    check_objective_weights(0.0, realism_weight, prior_weight, False)
    if not realism_weight > 0:
        raise ValueError("refinement follows the Discriminator's score: realism_weight must be > 0")


def _descend(eng, z, steps, lr, betas, grad, final_out=None):
    """The Adam-on-z loop of projection and refinement on one chunk: ``steps`` iterations of ``grad(k, z, dz, out)`` -- which
    writes the gradient at z into dz and the per-image objective into out (None: not wanted) -- and one Engine.op_adam on
    (z, dz, m, v), which updates ``z`` in place; then ``grad(steps, z, dz, final_out)``, the evaluation AT the returned z.
    Returns the (steps, b) history: the objective at the start of every iteration.  Nothing synchronises with the host."""
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    dz = torch.empty_like(z)
    hist = torch.empty(steps, z.shape[0], dtype=torch.float32, device=z.device)
    for k in range(steps):
        grad(k, z, dz, hist[k])
        eng.op_adam(z, dz, m, v, k + 1, lr=lr, beta1=betas[0], beta2=betas[1])
    grad(steps, z, dz, final_out)
    return hist


def _refine(eng, generator, z0, steps, lr, betas, realism_weight, prior_weight, despeckle=None):
    dev, latent = eng.device, eng.latent_dim
    z0 = torch.as_tensor(z0, dtype=torch.float32)
    if z0.dim() != 2 or z0.shape[1] != latent:
        raise ValueError(f"z0 must be (N, {latent}), got {tuple(z0.shape)}")
    n = z0.shape[0]
    z_all = z0.to(dev).contiguous().clone()
    before, after = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    hist = torch.empty(steps, n, dtype=torch.float32, device=dev)
    w = dict(realism_weight=realism_weight, prior_weight=prior_weight)
    for t0, b in refine_plan(n, eng.max_batch):
        z = z_all[t0:t0 + b]                                   # (a contiguous view: Adam updates the returned tensor in place)

        def grad(k, z, dz, out):
            ends = k == 0 or k == steps                        # the scores at z0 and AT the returned z
            res = eng.g_latent_objective_grad(z, want_probs=ends, dz_out=dz, objective_out=out, **w)
            if ends:
                (before if k == 0 else after)[t0:t0 + b] = res[2]

        hist[:, t0:t0 + b] = _descend(eng, z, steps, lr, betas, grad)
    size = eng.image_size
    u8 = np.empty((n, size, size), dtype=np.uint8)
    for t0, b in refine_plan(n, eng.max_batch):
        u8[t0:t0 + b] = generate_uint8(generator, z_all[t0:t0 + b], despeckle)
    return z_all, u8, before, after, hist


def refine_latents(generator: Generator, discriminator: Discriminator, z0: torch.Tensor, steps: int = 20, lr: float = 0.02,
                   betas: Tuple[float, float] = (0.9, 0.999), realism_weight: float = 1.0, prior_weight: float = 0.0):
    """Move the latent vectors ``z0`` (N, latent) towards images the Discriminator believes: ``steps`` iterations of Adam on z
    against the per-image objective realism_weight * -log D(G(z)) + prior_weight * 0.5 * mean(z^2), both networks in eval
    mode, every iteration one Engine.g_latent_objective_grad and one Engine.op_adam on (z, dz, m, v), in chunks of the
    engine's max_batch (refine_plan), all enqueued without a host synchronisation.  The Discriminator comes into the
    Generator's context by adopt_discriminator.

    Returns (z (N, latent) fp32 device tensor, images (N, S, S) uint8 numpy -- generate_uint8 at z --, probs_before (N,)
    device tensor: D(G(z0)), probs_after (N,): D(G(z)) at the returned z, history (steps, N) device tensor: the objective at
    the start of every iteration)."""
    _check_refine(steps, lr, realism_weight, prior_weight)
    eng = adopt_discriminator(generator, discriminator)
    return _refine(eng, generator, z0, steps, lr, betas, realism_weight, prior_weight)


def generate_signatures_refined(generator: Generator, discriminator: Discriminator, n_signatures: int, latent_dim: int,
                                device: torch.device, seed: Optional[int] = None, batch_size: int = 32, noise_scale: float = 1.0,
                                steps: int = 20, lr: float = 0.02, prior_weight: float = 0.0, threshold: Optional[int] = None,
                                despeckle: Optional[Despeckle] = None) -> Tuple[List[Any], List[float], List[float]]:
    """Generation with every latent vector refined by the Discriminator's score instead of oversampling and discarding:
    batch by batch (filter_plan with ratio 1.0: the same batches and seeds as generate_signatures_filtered draws first),
    z = randn * noise_scale, then refine_latents' loop.  Returns (PIL 'L' images in generation order -- binarised when
    ``threshold`` is given --, probs_after, probs_before): the scores D(G(z)) of the fp32 images after and before.
    ``despeckle``: the final bytes are cleaned before they are returned (the scores stay those of the fp32 images)."""
    from PIL import Image
    _check_refine(steps, lr, 1.0, prior_weight)
    if threshold is not None and not 0 <= int(threshold) <= 255:
        raise ValueError(f"threshold must be a byte value, got {threshold}")
    _, plan = filter_plan(n_signatures, 1.0, batch_size, seed)
    if not plan:
        return [], [], []
    eng = adopt_discriminator(generator, discriminator)
    images, before, after = [], [], []
    for b, batch_seed in plan:
        _seed_batch(batch_seed)
        z = torch.randn(b, latent_dim, device=device) * noise_scale
        _, u8, p0, p1, _ = _refine(eng, generator, z, steps, lr, (0.9, 0.999), 1.0, prior_weight, despeckle)
        if threshold is not None:
            u8 = binarize_uint8(u8, threshold)
        images += [Image.fromarray(arr, mode="L") for arr in u8]
        before.append(p0); after.append(p1)
    host = lambda ts: [float(x) for x in torch.cat(ts).cpu()]
    return images, host(after), host(before)


# ---- shape-attribute editing: slant, size, boldness, position ----------------------------------------------------------------
def check_edit(slant_delta=0.0, size_scale=1.0, boldness_scale=1.0, shift=(0.0, 0.0), steps=30, lr=0.02, keep_weight=1.0,
               realism_weight=0.0, prior_weight=0.0, shape_weight=1.0, has_discriminator=False):
    """The host-side refusals of edit_latents, raised as ValueError before anything is allocated.  Returns the edit as floats:
    (slant_delta, size_scale, boldness_scale, (dx, dy)).  Pure host code."""
    try:
        shift = tuple(float(v) for v in shift)
    except TypeError:
        shift = ()
    if len(shift) != 2:
        raise ValueError("shift must be two numbers (dx, dy)")
    edit = (float(slant_delta), float(size_scale), float(boldness_scale), shift)
    if not all(math.isfinite(v) for v in edit[:3] + shift):
        raise ValueError(f"the edit must be finite, got {edit}")
    if not edit[1] > 0 or not edit[2] > 0:
        raise ValueError(f"size_scale and boldness_scale must be > 0, got {edit[1]}, {edit[2]}")
    if edit == (0.0, 1.0, 1.0, (0.0, 0.0)):
        raise ValueError("no edit was asked for: give slant_delta != 0, size_scale != 1, boldness_scale != 1 or shift != (0, 0)")
    if steps < 1 or not lr > 0:
        raise ValueError(f"steps must be >= 1 and lr > 0, got {steps}, {lr}")
    w = (float(keep_weight), float(realism_weight), float(prior_weight), float(shape_weight))
    if any(not math.isfinite(x) or x < 0.0 for x in w):
        raise ValueError(f"keep_weight, realism_weight, prior_weight and shape_weight must be finite and >= 0, got {w}")
    if not w[3] > 0:
        raise ValueError("an edit follows the shape objective: shape_weight must be > 0")
    if w[1] > 0 and not has_discriminator:
        raise ValueError("realism_weight > 0 needs the Discriminator")
    return edit


def edit_targets(features0: torch.Tensor, slant_delta: float = 0.0, size_scale: float = 1.0, boldness_scale: float = 1.0,
                 shift: Tuple[float, float] = (0.0, 0.0), shape_weight: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(weights, targets), both fp64 (N, 8) where ``features0`` (N, 8) fp64 lives: what an edit asks of shape.shape_grad, from
    each start image's own features f0.  Targets: slant f0 + slant_delta; spread f0 * size_scale^2 (a signature R times as
    large has R^2 times the spread; sxx, syy and sxy get no target of their own); mass f0 * boldness_scale; cx f0 + dx and
    cy f0 + dy (``shift`` is one edit: both coordinates are held).  An edit left at its default gets weight 0 -- its target
    column holds f0 and is not looked at.  Weights: shape_weight / scale_k, so that one knob serves all: scale 1 for slant
    and the centre, max(f0_k^2, 1e-6) for mass and spread (their residuals are then relative).  Torch only, no
    synchronisation; works on the CPU."""
    from ..shape import CX, CY, MASS, SLANT, SPREAD
    f0 = features0
    if not isinstance(f0, torch.Tensor) or f0.dtype != torch.float64 or f0.dim() != 2 or f0.shape[1] != 8:
        raise ValueError("features0 must be a float64 (N, 8) tensor")
    w, t = torch.zeros_like(f0), f0.clone()
    def relative(k):                                           # (tensor / tensor: a correctly rounded division)
        scale = torch.clamp(f0[:, k] * f0[:, k], min=1e-6)
        return torch.full_like(scale, float(shape_weight)) / scale

    if slant_delta != 0.0:
        t[:, SLANT] = f0[:, SLANT] + float(slant_delta)
        w[:, SLANT] = float(shape_weight)
    if size_scale != 1.0:
        t[:, SPREAD] = f0[:, SPREAD] * (float(size_scale) * float(size_scale))
        w[:, SPREAD] = relative(SPREAD)
    if boldness_scale != 1.0:
        t[:, MASS] = f0[:, MASS] * float(boldness_scale)
        w[:, MASS] = relative(MASS)
    if tuple(shift) != (0.0, 0.0):
        t[:, CX], t[:, CY] = f0[:, CX] + float(shift[0]), f0[:, CY] + float(shift[1])
        w[:, CX] = w[:, CY] = float(shape_weight)
    return w.contiguous(), t.contiguous()


def edit_latents(generator: Generator, z0: torch.Tensor, slant_delta: float = 0.0, size_scale: float = 1.0,
                 boldness_scale: float = 1.0, shift: Tuple[float, float] = (0.0, 0.0), steps: int = 30, lr: float = 0.02,
                 betas: Tuple[float, float] = (0.9, 0.999), keep_weight: float = 1.0, discriminator: Optional[Discriminator] = None,
                 realism_weight: float = 0.0, prior_weight: float = 0.0, shape_weight: float = 1.0):
    """Move the latent vectors ``z0`` (N, latent) so that their signatures lean more (``slant_delta`` is added to the slant; a
    NEGATIVE delta leans to the right, because the image's v axis points down), sit larger in the frame (``size_scale`` R: the
    spread becomes R^2 times what it is), carry more ink (``boldness_scale``: the mass is multiplied) or move (``shift``
    (dx, dy) in units of the image side, dy downwards) -- while staying the same signature.  The shape objective is
    shape.shape_grad's with edit_targets' weights and targets, from each start image's own features f0 = shape(G(z0));
    staying the same is the reconstruction term keep_weight * mean((G(z) - t0)^2) against the bytes t0 generate_uint8 gives at
    z0; ``realism_weight`` (needs ``discriminator``, brought in by adopt_discriminator) and ``prior_weight`` are refine_latents'.

    ``steps`` iterations of Adam on z, every iteration Engine.g_forward(z) -> shape.shape_grad (the image-space gradient of the
    shape objective at G(z)) -> the seeded Engine.g_latent_objective_grad (J_G^T of it joins dz) -> the shape objective added
    in torch -> Engine.op_adam, in chunks of the engine's max_batch (refine_plan), all enqueued without a host
    synchronisation.  The Generator must be in eval() mode; its weights and BatchNorm buffers do not move.

    Returns (z (N, latent) fp32 device tensor, images (N, S, S) uint8 numpy -- generate_uint8 at z --, features_before (N, 8)
    fp64 device tensor, features_after (N, 8): at the returned z, targets (N, 8): edit_targets' (a column without an edit holds
    f0), history (steps + 1, N) fp32 device tensor: the full objective at the start of every iteration and, last, AT the
    returned z).  A call that asks for no edit raises ValueError.  Whether an edit reaches its target depends on the
    Generator; nothing here promises it."""
    from ..shape import _shape_grad_checked, shape_features
    edit = check_edit(slant_delta, size_scale, boldness_scale, shift, steps, lr, keep_weight, realism_weight, prior_weight,
                      shape_weight, discriminator is not None)
    if generator.training:
        raise ValueError("edit_latents needs the Generator in eval() mode (running BatchNorm statistics)")
    eng = adopt_discriminator(generator, discriminator) if realism_weight > 0 else generator._require_engine()
    dev, latent, size = eng.device, eng.latent_dim, eng.image_size
    z0 = torch.as_tensor(z0, dtype=torch.float32)
    if z0.dim() != 2 or z0.shape[1] != latent:
        raise ValueError(f"z0 must be (N, {latent}), got {tuple(z0.shape)}")
    n = z0.shape[0]
    z_all = z0.to(dev).contiguous().clone()
    before, after, targets = (torch.empty(n, 8, dtype=torch.float64, device=dev) for _ in range(3))
    hist = torch.empty(steps + 1, n, dtype=torch.float32, device=dev)
    for t0, b in refine_plan(n, eng.max_batch):
        z = z_all[t0:t0 + b]                                   # (a contiguous view: Adam updates the returned tensor in place)
        f0 = shape_features(eng.g_forward(z, training=False))
        w, t = edit_targets(f0, *edit, shape_weight=shape_weight)
        before[t0:t0 + b], targets[t0:t0 + b] = f0, t
        keep = eng.g_generate_u8(z) if keep_weight > 0 else None
        dx = torch.empty(b, 1, size, size, dtype=torch.float32, device=dev)
        shape_obj = torch.empty(b, dtype=torch.float32, device=dev)

        def grad(k, z, dz, out):
            img = eng.g_forward(z, training=False)
            feats = _shape_grad_checked(img, b, size, dev, w, t, dx, shape_obj)[2]
            eng.g_latent_objective_grad(z, keep, keep_weight, realism_weight, prior_weight, dz_out=dz, objective_out=out, image_grad=dx)
            out += shape_obj
            if k == steps:
                after[t0:t0 + b] = feats

        hist[:steps, t0:t0 + b] = _descend(eng, z, steps, lr, betas, grad, hist[steps, t0:t0 + b])
    u8 = np.empty((n, size, size), dtype=np.uint8)
    for t0, b in refine_plan(n, eng.max_batch):
        u8[t0:t0 + b] = generate_uint8(generator, z_all[t0:t0 + b])
    return z_all, u8, before, after, targets, hist


def generate_signatures_edited(generator: Generator, n_signatures: int, latent_dim: int, device: torch.device,
                               seed: Optional[int] = None, batch_size: int = 32, noise_scale: float = 1.0,
                               threshold: Optional[int] = None, **edit) -> Tuple[List[Any], List[Dict[str, Any]]]:
    """Generation with every latent vector edited (edit_latents; ``edit``: its keyword arguments) before its image is made.
    The latent vectors are the ones generate_signatures_batch draws for the same ``seed``, ``batch_size`` and ``noise_scale``
    (one seeding, then z = randn * noise_scale per batch; the edit draws nothing), so image i of this run is the edited
    image i of the plain run.  Returns (PIL 'L' images in generation order -- binarised when ``threshold`` is given --,
    records): per image {before, targets, after} -- the eight features by name, ``targets`` only those the edit weighs --
    and {objective_before, objective_after}, the ends of the objective's history."""
    from PIL import Image
    from ..shape import CX, CY, FEATURES, MASS, SLANT, SPREAD
    if threshold is not None and not 0 <= int(threshold) <= 255:
        raise ValueError(f"threshold must be a byte value, got {threshold}")
    asked = check_edit(**{k: v for k, v in edit.items() if k not in ("betas", "discriminator")},
                       has_discriminator=edit.get("discriminator") is not None)
    edited = sorted(([SLANT] if asked[0] != 0.0 else []) + ([SPREAD] if asked[1] != 1.0 else [])
                    + ([MASS] if asked[2] != 1.0 else []) + ([CX, CY] if asked[3] != (0.0, 0.0) else []))
    _seed_batch(seed)
    images, records, done = [], [], 0
    while done < n_signatures:
        b = min(batch_size, n_signatures - done)
        z = torch.randn(b, latent_dim, device=device) * noise_scale
        _, u8, before, after, targets, hist = edit_latents(generator, z, **edit)
        if threshold is not None:
            u8 = binarize_uint8(u8, threshold)
        images += [Image.fromarray(arr, mode="L") for arr in u8]
        before, after, targets, hist = before.cpu().numpy(), after.cpu().numpy(), targets.cpu().numpy(), hist.cpu().numpy()
        for i in range(b):
            named = lambda row, ks=range(8): {FEATURES[k]: float(row[k]) for k in ks}          # noqa: E731
            records.append({"before": named(before[i]), "targets": named(targets[i], edited), "after": named(after[i]),
                            "objective_before": float(hist[0, i]), "objective_after": float(hist[-1, i])})
        done += b
    return images, records


def check_identity_projection(generator, verifier, identity_weight, identity_score_weight, verifier_resize=False):
    """The host-side refusals of project_signatures' identity term, raised as ValueError before anything is allocated.
    Returns None when both weights are 0 -- the verifier is then not looked at -- else the two weights as floats.
    ``verifier_resize``: the verifier reads G(z) through the device resize, so the Generator need not be a 64x64 one."""
    w = (float(identity_weight), float(identity_score_weight))
    if any(not math.isfinite(x) or x < 0.0 for x in w):
        raise ValueError(f"the identity weights must be finite and >= 0, got {w}")
    if w == (0.0, 0.0):
        return None
    if verifier is None:
        raise ValueError("identity_weight / identity_score_weight > 0 need the verifier")
    if generator.output_size != 64 and not verifier_resize:
        raise ValueError(f"the verifier reads 64x64 images: the identity term needs a 64x64 Generator, got {generator.output_size}")
    if verifier.training:
        raise ValueError("the identity term runs the verifier in eval mode: call .eval() on it")
    g_dev, v_dev = next(generator.parameters()).device, next(verifier.parameters()).device
    if g_dev != v_dev:
        raise ValueError(f"the verifier lives on {v_dev}, the Generator on {g_dev}: move them to one device")
    return w


def _identity_grad(eng, verifier, t, ref_emb, realism_weight, prior_weight, w_e, w_s, resize=False):
    """The ``grad`` of _descend with the identity term: g_forward -> verifier.input_grad (the image-space gradient of the
    identity objective at G(z)) -> the seeded latent call (J_G^T of it joins dz) -> the identity objective added in torch.
    ``resize``: verifier.input_grad_resized instead, which is input_grad itself at 64x64."""
    b = t.shape[0]
    input_grad = verifier.input_grad_resized if resize else verifier.input_grad
    dx = torch.empty(b, 1, eng.image_size, eng.image_size, dtype=torch.float32, device=eng.device)
    ident = torch.empty(b, dtype=torch.float32, device=eng.device)

    def grad(k, z, dz, out):
        img = eng.g_forward(z, training=False)
        input_grad(img, ref_emb, w_e, w_s, dx_out=dx, objective_out=ident)
        eng.g_latent_objective_grad(z, t, 1.0, realism_weight, prior_weight, dz_out=dz, objective_out=out, image_grad=dx)
        if out is not None:
            out += ident
    return grad


def project_signatures(generator: Generator, targets_u8, steps: int = 200, lr: float = 0.05,
                       betas: Tuple[float, float] = (0.9, 0.999), z0: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                       restarts: int = 1, return_candidates: bool = False, discriminator: Optional[Discriminator] = None,
                       realism_weight: float = 0.0, prior_weight: float = 0.0, verifier=None, identity_weight: float = 0.0,
                       identity_score_weight: float = 0.0, verifier_resize: bool = False):
    """Latent vectors whose images reproduce ``targets_u8`` ((N, S, S) uint8, numpy or tensor; a byte stands for
    byte / 127.5 - 1.0): ``steps`` iterations of Adam on z against the per-image loss mean((G(z) - t)^2), every iteration one
    Engine.g_latent_objective_grad (eval forward + eval backward in HIP) and one Engine.op_adam on (z, dz, m, v), all enqueued
    without a host synchronisation.  The Generator must be in eval() mode.  Batches: projection_plan; starts: projection_starts.

    Returns (z (N, latent) fp32 device tensor, recon (N, S, S) uint8 numpy -- generate_uint8 at z --, loss (N,) device tensor:
    the loss AT the returned z, history (steps, N) device tensor: the loss at the start of every iteration).  With
    ``restarts`` > 1 each target keeps the start whose final loss is lowest (the first of equals); ``return_candidates`` adds
    a dict with every candidate's ``z`` (R, N, latent), ``loss`` (R, N) and ``history`` (R, steps, N), and the kept ``choice``.

    ``realism_weight`` / ``prior_weight`` > 0 add realism_weight * -log D(G(z)) (needs ``discriminator``, brought in by
    adopt_discriminator) and prior_weight * 0.5 * mean(z^2) to the pixel error, and loss / history hold that objective.  With
    the defaults the weights are (1, 0, 0): the Discriminator is not run, and every bit is Engine.g_latent_grad's.

    ``identity_weight`` / ``identity_score_weight`` > 0 add the Siamese ``verifier``'s (signature_verifier_eval.SiameseNetwork,
    eval mode, the Generator's device; 64x64 Generators only) judgement that G(z) is the target's hand: identity_weight *
    0.5 * |e(G(z)) - e(t)|^2 + identity_score_weight * -log s(e(G(z)), e(t)).  The targets are embedded once (embed_u8);
    every iteration is then Engine.g_forward -> verifier.input_grad -> the seeded Engine.g_latent_objective_grad -> op_adam,
    still without a host synchronisation, and loss / history hold the full objective (restart selection uses it).  With both
    weights 0 the verifier is never touched and every bit is as without these arguments.

    ``verifier_resize``: the verifier reads the targets and G(z) through the device resize to 64x64 (Pillow's antialiased
    bilinear filter, resize.py: embed_resized for the targets' bytes, input_grad_resized -- resize_f32, input_grad, the
    resize's transpose -- for G(z)), so a 128x128 Generator can take the identity term.  On a 64x64 Generator it changes no bit."""
    identity = check_identity_projection(generator, verifier, identity_weight, identity_score_weight, verifier_resize)
    if generator.training:
        raise ValueError("project_signatures needs the Generator in eval() mode (running BatchNorm statistics)")
    if steps < 1 or restarts < 1:
        raise ValueError(f"steps and restarts must be >= 1, got {steps}, {restarts}")
    from ..engine import check_objective_weights
    check_objective_weights(1.0, realism_weight, prior_weight, True)
    if realism_weight > 0 and discriminator is None:
        raise ValueError("realism_weight > 0 needs the Discriminator")
    eng = adopt_discriminator(generator, discriminator) if realism_weight > 0 else generator._require_engine()
    dev, latent, size = eng.device, eng.latent_dim, eng.image_size
    t_all = torch.as_tensor(np.ascontiguousarray(targets_u8) if isinstance(targets_u8, np.ndarray) else targets_u8)
    if t_all.dtype != torch.uint8 or t_all.dim() != 3 or tuple(t_all.shape[1:]) != (size, size):
        raise ValueError(f"targets_u8 must be uint8 (N, {size}, {size}), got {t_all.dtype} {tuple(t_all.shape)}")
    t_all = t_all.to(dev).contiguous()
    n = t_all.shape[0]
    cand_z = torch.empty(restarts, n, latent, dtype=torch.float32, device=dev)
    cand_loss = torch.empty(restarts, n, dtype=torch.float32, device=dev)
    cand_hist = torch.empty(restarts, steps, n, dtype=torch.float32, device=dev)
    starts = {}
    for r, t0, b in projection_plan(n, restarts, eng.max_batch):
        if r not in starts:
            starts[r] = projection_starts(n, latent, r, z0, seed).to(dev)
        z = starts[r][t0:t0 + b].contiguous().clone()
        t = t_all[t0:t0 + b]
        grad = lambda k, z, dz, out: eng.g_latent_objective_grad(z, t, 1.0, realism_weight, prior_weight, dz_out=dz, objective_out=out)
        if identity:
            ref_emb = verifier.embed_resized(t) if verifier_resize else verifier.embed_u8(t)
            grad = _identity_grad(eng, verifier, t, ref_emb, realism_weight, prior_weight, *identity, resize=bool(verifier_resize))
        cand_hist[r, :, t0:t0 + b] = _descend(eng, z, steps, lr, betas, grad, cand_loss[r, t0:t0 + b])  # (the loss at the returned z)
        cand_z[r, t0:t0 + b] = z
    choice = torch.argmin(cand_loss, dim=0)                                        # (plumbing: the first of equal minima)
    pick = torch.arange(n, device=dev)
    z_best, loss_best, hist_best = cand_z[choice, pick], cand_loss[choice, pick], cand_hist[choice, :, pick].t().contiguous()
    recon = np.empty((n, size, size), dtype=np.uint8)
    for t0 in range(0, n, eng.max_batch):
        recon[t0:t0 + eng.max_batch] = generate_uint8(generator, z_best[t0:t0 + eng.max_batch].contiguous())
    out = (z_best, recon, loss_best, hist_best)
    if return_candidates:
        out += ({"z": cand_z, "loss": cand_loss, "history": cand_hist, "choice": choice},)
    return out


# ---- few-shot adaptation of the Generator's weights (pivotal tuning) --------------------------------------------------------
def adaptation_plan(first_layer: int, n_blocks: int) -> Tuple[List[str], List[str]]:
    """(trainable state_dict keys, frozen keys) of an adaptation that trains layers >= ``first_layer`` (layout.adaptation_plan:
    layer 0 fc, 1 .. n_blocks the upsample blocks, n_blocks + 1 the final conv).  Pure host code."""
    from .. import layout
    return layout.adaptation_plan(first_layer, n_blocks)


def _check_adapt(steps, lr, first_layer, n_blocks, anchor_weight, realism_weight):
    import math
    from ..engine import check_objective_weights
    if steps < 1 or not lr > 0:
        raise ValueError(f"steps must be >= 1 and lr > 0, got {steps}, {lr}")
    adaptation_plan(first_layer, n_blocks)
    if not math.isfinite(float(anchor_weight)) or anchor_weight < 0:
        raise ValueError(f"anchor_weight must be finite and >= 0, got {anchor_weight}")
    check_objective_weights(1.0, realism_weight, 0.0, True)


def adapt_generator(generator: Generator, targets_u8, z: Optional[torch.Tensor] = None, steps: int = 100, lr: float = 1e-4,
                    betas: Tuple[float, float] = (0.9, 0.999), first_layer: int = 0, anchor_weight: float = 0.0,
                    discriminator: Optional[Discriminator] = None, realism_weight: float = 0.0,
                    project_kwargs: Optional[Dict[str, Any]] = None, seed: Optional[int] = None) -> Dict[str, Any]:
    """Adapt the Generator's WEIGHTS to a few target signatures ``targets_u8`` ((N, S, S) uint8, N <= the engine's max_batch) --
    pivotal tuning: the pivots are ``z`` (N, latent), or project_signatures(generator, targets_u8, seed=seed, **project_kwargs)
    when ``z`` is None; they stay fixed while Adam runs on the parameters of layers >= ``first_layer`` (adaptation_plan) against
    mean((G(z) - t)^2) + realism_weight * -log D(G(z)), both networks in eval mode: BatchNorm stays the affine of its running
    statistics, which do not move.  Every iteration is one Engine.g_param_grad, Engine.op_anchor (``anchor_weight`` != 0: the
    pull anchor_weight * (theta - theta0) back to the starting weights), Engine.op_adam on the trainable suffix of the arena
    with the loop's own moments and grad_scale = 1 / N, and Engine.params_changed(); nothing synchronises with the host.

    The Generator's parameters are changed IN PLACE.  Returns a dict: ``z`` the pivots (device), ``history`` (steps, N) the
    objective at the start of every iteration, ``loss_before`` / ``loss_after`` (N,) device tensors (history[0]; the
    objective at the adapted weights), ``recon`` (N, S, S) uint8 numpy -- generate_uint8 at the pivots --, ``snapshot`` a
    device copy of the parameters before the first update (restore_generator puts them back), ``trainable`` the keys."""
    if generator.training:
        raise ValueError("adapt_generator needs the Generator in eval() mode (running BatchNorm statistics)")
    eng = generator._require_engine()
    _check_adapt(steps, lr, first_layer, eng.g_layers, anchor_weight, realism_weight)
    if realism_weight > 0 and discriminator is None:
        raise ValueError("realism_weight > 0 needs the Discriminator")
    dev, latent, size = eng.device, eng.latent_dim, eng.image_size
    t = torch.as_tensor(np.ascontiguousarray(targets_u8) if isinstance(targets_u8, np.ndarray) else targets_u8)
    if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape[1:]) != (size, size):
        raise ValueError(f"targets_u8 must be uint8 (N, {size}, {size}), got {t.dtype} {tuple(t.shape)}")
    n = t.shape[0]
    if n < 1 or n > eng.max_batch:
        raise ValueError(f"adaptation is few-shot: 1 <= N <= max_batch = {eng.max_batch} targets in one batch, got {n}")
    if z is None:
        z = project_signatures(generator, t, seed=seed, **(project_kwargs or {}))[0]
    z = torch.as_tensor(z, dtype=torch.float32).to(dev).contiguous().clone()
    if tuple(z.shape) != (n, latent):
        raise ValueError(f"z must be ({n}, {latent}), got {tuple(z.shape)}")
    if realism_weight > 0:
        eng = adopt_discriminator(generator, discriminator)
    t = t.to(dev).contiguous()
    off, num = eng.layer_span(first_layer)
    snapshot = eng.g_params.clone()
    p, p0 = eng.g_params[off:off + num], snapshot[off:off + num]
    dparams = torch.empty_like(eng.g_params)
    g = dparams[off:off + num]
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    hist = torch.empty(steps, n, dtype=torch.float32, device=dev)
    after = torch.empty(n, dtype=torch.float32, device=dev)
    grad = lambda out: eng.g_param_grad(z, t, 1.0, realism_weight, first_layer, dparams_out=dparams, objective_out=out)
    for k in range(steps):
        grad(hist[k])
        if anchor_weight != 0:
            eng.op_anchor(g, p, p0, anchor_weight)
        eng.op_adam(p, g, m, v, k + 1, lr=lr, beta1=betas[0], beta2=betas[1], grad_scale=1.0 / n)
        eng.params_changed()
    grad(after)
    return {"z": z, "history": hist, "loss_before": hist[0].clone(), "loss_after": after, "recon": generate_uint8(generator, z),
            "snapshot": snapshot, "trainable": adaptation_plan(first_layer, eng.g_layers)[0]}


def restore_generator(generator: Generator, snapshot: torch.Tensor) -> None:
    """Put the parameters adapt_generator saved (its ``snapshot``) back into the Generator's arena."""
    eng = generator._require_engine()
    if snapshot.shape != eng.g_params.shape or snapshot.dtype != torch.float32:
        raise ValueError(f"snapshot must be the float32 ({eng.g_params.numel()},) tensor adapt_generator returned")
    with torch.no_grad():
        eng.g_params.copy_(snapshot.to(eng.device))
    eng.params_changed()


def morph_blend(z_a: torch.Tensor, z_b: torch.Tensor, n_frames: int) -> torch.Tensor:
    """(n_frames, latent): frame i is (1 - a) * z_a + a * z_b with a = i / (n_frames - 1), the app's expression
    (app_vanilla_gan_signatures.py:1696-1697) evaluated frame by frame in fp32 on the endpoints' device.  The endpoints are
    (1, latent) or (latent,) -- the app draws them as (1, latent, 1, 1), which its own nn.Linear rejects."""
    if n_frames < 2:
        raise ValueError(f"n_frames must be >= 2, got {n_frames}")
    z_a, z_b = z_a.reshape(1, -1).float(), z_b.reshape(1, -1).float()
    if z_a.shape != z_b.shape:
        raise ValueError(f"endpoints differ in shape: {tuple(z_a.shape)} vs {tuple(z_b.shape)}")
    frames = []
    for i in range(n_frames):
        a = i / (n_frames - 1)
        frames.append((1 - a) * z_a + a * z_b)
    return torch.cat(frames, dim=0)


def morph_sequence(generator: Generator, z_a: torch.Tensor, z_b: torch.Tensor, n_frames: int) -> np.ndarray:
    """(n_frames, S, S) uint8: the frames of the app's "Export Morph Sequence" between two latent endpoints, blended on the
    device (morph_blend) and generated as bytes by the Generator's last kernel -- one latent vector per forward, as the app
    generates them, so a frame's bytes are generate_uint8's at that vector whatever the number of frames (the library picks
    its kernels by batch size); the frames land in one pool on the device and cross to the host together.  Deliberate
    deviation: a frame's bytes follow this project's rule (tensor_to_uint8: (x + 1) * 127.5, clip, truncate), not the tab's
    ((x + 1) / 2).clamp(0, 1) * 255."""
    if generator.training:
        raise ValueError("morph_sequence needs the Generator in eval() mode")
    eng = generator._require_engine()
    z = morph_blend(z_a.to(eng.device), z_b.to(eng.device), n_frames)
    pool = torch.empty(n_frames, eng.image_size, eng.image_size, dtype=torch.uint8, device=eng.device)
    for i in range(n_frames):
        eng.g_generate_u8(z[i:i + 1].contiguous(), out=pool[i:i + 1])
    return _to_host_u8(pool)


def morph_strip(frames, threshold: Optional[int] = None, make_transparent: bool = False):
    """The frames side by side as one PIL image, laid out as the app does (app_vanilla_gan_signatures.py:1706-1712): an 'L'
    canvas of 255 -- or with ``make_transparent`` an 'RGBA' canvas of (255, 255, 255, 0) --, every frame converted to the
    canvas' mode and pasted at x = i * width.  ``frames``: (n, H, W) uint8 or PIL images; with a ``threshold`` each goes
    through process_images first (the app's apply_threshold), which is also what ``make_transparent`` acts through."""
    from PIL import Image
    images = [f if isinstance(f, Image.Image) else Image.fromarray(np.asarray(f, dtype=np.uint8), mode="L") for f in frames]
    if not images:
        raise ValueError("morph_strip needs at least one frame")
    if threshold is not None:
        images = process_images(images, threshold=threshold, make_transparent=make_transparent)
    w, h = images[0].width, images[0].height
    strip = Image.new("RGBA" if make_transparent else "L", (w * len(images), h), (255, 255, 255, 0) if make_transparent else 255)
    for i, frame in enumerate(images):
        if frame.mode != strip.mode:
            frame = frame.convert(strip.mode)
        strip.paste(frame, (i * w, 0))
    return strip
