"""Drop-in for the reference's ``utils/inference.py`` (checkpoint -> Generator, batched generation,
tensor -> PIL) on the MI355X HIP engine.

Checkpoint tolerance is the reference's (utils/inference.py:20-104): a dict with
``generator_state_dict`` (trainer layout A / VanillaGAN layout B), a dict with ``state_dict``, or a
bare Generator state_dict whose architecture is inferred from ``fc.*weight.shape[1]`` and the count
of ``upsample_blocks.N.block.0.weight`` keys (>= 5 -> 128x128)."""
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

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
