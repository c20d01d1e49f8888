"""Drop-in for the reference's ``utils/inference.py`` (checkpoint -> Generator, batched generation,
tensor -> PIL) on the MI355X HIP engine.

Checkpoint tolerance is the reference's (utils/inference.py:20-104): a dict with
``generator_state_dict`` (trainer layout A / VanillaGAN layout B), a dict with ``state_dict``, or a
bare Generator state_dict whose architecture is inferred from ``fc.*weight.shape[1]`` and the count
of ``upsample_blocks.N.block.0.weight`` keys (>= 5 -> 128x128).

Realism-filtered generation (the reference app's "Filter by Realism", app_vanilla_gan_signatures.py:1065-1385, which is not UI:
it is where a trained Discriminator is used after training) lives here too: ``load_discriminator``, ``binarize_uint8`` /
``process_images``, ``filter_plan`` and ``generate_signatures_filtered``."""
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


def generate_uint8(generator: Generator, z: torch.Tensor) -> np.ndarray:
    """z (B, latent) -> (B, H, W) uint8, the bytes of ``tensor_to_uint8(generator(z))``.  In eval mode the Generator's last
    kernel writes them itself (Engine.g_generate_u8) and one byte per pixel crosses to the host; a Generator left in train()
    mode (BatchNorm batch statistics) has no such kernel and takes the fp32 route."""
    if generator.training:
        return tensor_to_uint8(generator(z))
    return _to_host_u8(generator._require_engine().g_generate_u8(z))


def tensor_to_pil_image(tensor: torch.Tensor):
    from PIL import Image
    return Image.fromarray(tensor_to_uint8(tensor.unsqueeze(0))[0], mode="L")


def generate_signatures_batch(generator: Generator, n_samples: int, latent_dim: int, device: torch.device,
                              seed: Optional[int] = None, batch_size: int = 32, progress_callback=None,
                              noise_scale: float = 1.0) -> List[Any]:
    """Reference semantics (utils/inference.py:136-194): optional torch.manual_seed, then per batch
    z = randn(b, latent, device=device) * noise_scale -> generator(z) -> one PIL image per sample."""
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
        for arr in generate_uint8(generator, z):
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


def generate_signatures_filtered(generator: Generator, discriminator: Discriminator, n_signatures: int, latent_dim: int,
                                 device: torch.device, seed: Optional[int] = None, batch_size: int = 32,
                                 oversampling_ratio: float = 2.0, noise_scale: float = 1.0, threshold: Optional[int] = None,
                                 route: str = "device", progress_callback=None) -> Tuple[List[Any], List[float]]:
    """The reference app's "Filter by Realism": generate int(n * ratio) signatures batch by batch (filter_plan), binarise them
    when ``threshold`` is given, score each with the Discriminator on byte / 127.5 - 1.0, and return the best min(n, total)
    as (PIL 'L' images, scores), highest score first, equal scores in generation order.

    route="device": the bytes go from the Generator's last kernel into a pool in HBM, the Discriminator's first block reads
    them there (Engine.d_score_u8) and writes into the pool's score vector; after the last batch one select_topk and one
    gather_u8 run, and only the selected images and scores cross to the host.  route="host": the reference's loop on the
    existing pieces -- bytes to the host, numpy binarisation, CPU dequantisation, Discriminator.forward, Python's sort.  Both
    give identical images and scores.  The device route falls back to the host route where it does not apply: a Generator or
    Discriminator in train() mode, or more than _lib.SELECT_MAX images."""
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
            if threshold is not None:
                u8 = binarize_uint8(u8, threshold)
            with torch.no_grad():
                scores = discriminator(dequantize_uint8(u8).to(device)).cpu().numpy().flatten().tolist()
            records += [(arr, float(sc)) for arr, sc in zip(u8, scores)]
            tick(b)
        records.sort(key=lambda r: r[1], reverse=True)
        records = records[:keep]
        return [Image.fromarray(arr, mode="L") for arr, _ in records], [sc for _, sc in records]

    g_eng, d_eng = generator._require_engine(), discriminator._require_engine()
    size = g_eng.image_size
    pool = torch.empty(total, size, size, dtype=torch.uint8, device=g_eng.device)
    scores = torch.empty(total, dtype=torch.float32, device=g_eng.device)
    binarize = None if threshold is None else int(threshold)
    for b, batch_seed in plan:
        _seed_batch(batch_seed)
        z = torch.randn(b, latent_dim, device=device) * noise_scale
        g_eng.g_generate_u8(z, out=pool[done:done + b])
        d_eng.d_score_u8(pool[done:done + b], binarize=binarize, out=scores[done:done + b])
        tick(b)
    index = g_eng.select_topk(scores, keep)
    picked = _to_host_u8(g_eng.gather_u8(pool, index, binarize=binarize))
    best = _to_host_u8(scores[index.long()].view(torch.uint8)).view(np.float32)
    return [Image.fromarray(arr, mode="L") for arr in picked], [float(sc) for sc in best]
