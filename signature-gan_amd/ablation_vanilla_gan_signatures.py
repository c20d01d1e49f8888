"""Drop-in for the training parts of the reference's ``ablation_vanilla_gan_signatures`` on the MI355X HIP engine.

``ConfigurableGenerator`` (ablation_vanilla_gan_signatures.py:216-328, with UpsampleBlockConfigurable :159-213) is the
reference Generator with ReLU or LeakyReLU after every BatchNorm; the activation runs inside the same HIP kernels as the
ReLU network (``siggan_config.g_leaky_slope``).  ``AblationConfig`` / ``AblationResult`` are the reference's plain
dataclasses (:51-157), and ``AblationGANTrainer`` (:335-532) runs its ``train_epoch`` iteration through
``Engine.ablation_step`` (the library's SIGGAN_STEP_ABLATION variant).  The study manager (tables, plots, FID) is not
mirrored."""
import time
from dataclasses import asdict, dataclass, field
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .discriminator_vanilla_gan import Discriminator
from .engine import Engine
from .generator_vanilla_gan import Generator
from ._modules import EngineAdam


@dataclass
class AblationConfig:
    """One ablation experiment (ablation_vanilla_gan_signatures.py:51-95)."""
    name: str
    latent_dim: int = 100
    activation: str = "relu"  # 'relu' or 'leaky_relu'
    use_spectral_norm: bool = False
    image_size: int = 64
    image_channels: int = 1
    batch_size: int = 64
    epochs: int = 50
    g_lr: float = 2e-4
    d_lr: float = 2e-4
    beta1: float = 0.5
    beta2: float = 0.999
    label_smoothing: float = 0.9

    def to_dict(self) -> Dict[str, Any]:
        return asdict(self)

    def get_short_name(self) -> str:
        spec_str = "SN" if self.use_spectral_norm else "noSN"
        act_str = "LReLU" if self.activation == "leaky_relu" else "ReLU"
        return f"z{self.latent_dim}_{act_str}_{spec_str}"


@dataclass
class AblationResult:
    """Results of one experiment (ablation_vanilla_gan_signatures.py:96-157); ``fid_score`` stays None (no Inception)."""
    config: AblationConfig
    g_losses: List[float] = field(default_factory=list)
    d_losses: List[float] = field(default_factory=list)
    d_real_scores: List[float] = field(default_factory=list)
    d_fake_scores: List[float] = field(default_factory=list)
    fid_score: Optional[float] = None
    loss_variance_g: float = 0.0
    loss_variance_d: float = 0.0
    final_g_loss: float = 0.0
    final_d_loss: float = 0.0
    training_time: float = 0.0
    sample_path: str = ""

    def compute_stability_metrics(self) -> None:
        if self.g_losses:
            self.loss_variance_g = float(np.var(self.g_losses))
            self.final_g_loss = self.g_losses[-1]
        if self.d_losses:
            self.loss_variance_d = float(np.var(self.d_losses))
            self.final_d_loss = self.d_losses[-1]

    def to_dict(self) -> Dict[str, Any]:
        return {
            "config": self.config.to_dict(),
            "g_losses": self.g_losses,
            "d_losses": self.d_losses,
            "d_real_scores": self.d_real_scores,
            "d_fake_scores": self.d_fake_scores,
            "fid_score": self.fid_score,
            "loss_variance_g": self.loss_variance_g,
            "loss_variance_d": self.loss_variance_d,
            "final_g_loss": self.final_g_loss,
            "final_d_loss": self.final_d_loss,
            "training_time": self.training_time,
            "sample_path": self.sample_path,
        }


class ConfigurableGenerator(Generator):
    """The reference's ConfigurableGenerator: same constructor, attributes and ``state_dict`` keys as ``Generator`` (the
    activations hold no state).  ``activation == "leaky_relu"`` selects LeakyReLU(``leaky_slope``) after every BatchNorm;
    any other value means ReLU, as in the reference (:198-201, :283-286)."""

    def __init__(self, latent_dim: int = 100, output_size: int = 64, output_channels: int = 1, base_features: int = 256,
                 activation: str = "relu", leaky_slope: float = 0.2, _engine=None) -> None:
        super().__init__(latent_dim=latent_dim, output_size=output_size, output_channels=output_channels,
                         base_features=base_features)
        self.activation = activation
        self.leaky_slope = float(leaky_slope)
        if _engine is not None:
            if _engine.g_activation != self._g_activation() or (
                    self._g_activation() == "leaky_relu" and abs(_engine.g_slope - self.leaky_slope) > 1e-12):
                raise ValueError("shared engine was created with a different Generator activation / leaky_slope")
            self._shared_engine = True
            self._attach(_engine, copy_in=True)

    def _g_activation(self):
        return "leaky_relu" if self.activation == "leaky_relu" else "relu"

    def _engine_kwargs(self):
        return dict(latent_dim=self.latent_dim, image_size=self.output_size, g_activation=self._g_activation(),
                    g_leaky_slope=self.leaky_slope)


class AblationGANTrainer:
    """AblationGANTrainer (ablation_vanilla_gan_signatures.py:335-532) on one shared engine in the ablation step variant:
    each iteration of ``train_epoch`` is one ``Engine.ablation_step`` (both networks in train mode, one Generator forward,
    the G update against the smoothed real label).  ``data_loader``: any iterable of (B, 1, S, S) tensors or of tuples whose
    first element is one.  z and the dropout masks come from the engine's RNG (seeded from torch's global generator)."""

    def __init__(self, config: AblationConfig, data_loader, device, output_dir) -> None:
        self.config = config
        self.data_loader = data_loader
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("AblationGANTrainer (HIP engine) needs a ROCm device; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.output_dir = Path(output_dir)
        g_act = "leaky_relu" if config.activation == "leaky_relu" else "relu"
        self.engine = Engine(latent_dim=config.latent_dim, image_size=config.image_size, max_batch=config.batch_size,
                             device=str(self.device), seed=torch.initial_seed() & ((1 << 63) - 1),
                             image_channels=config.image_channels, spectral_norm=config.use_spectral_norm,
                             g_activation=g_act)
        self.generator = ConfigurableGenerator(latent_dim=config.latent_dim, output_size=config.image_size,
                                               output_channels=config.image_channels, activation=config.activation,
                                               _engine=self.engine)
        self.discriminator = Discriminator(input_size=config.image_size, input_channels=config.image_channels,
                                           use_spectral_norm=config.use_spectral_norm, _engine=self.engine)
        self.engine.set_step_variant("ablation")
        self.criterion = nn.BCELoss()            # kept for API parity; the loss is fused in the engine
        self.g_optimizer = EngineAdam(self.generator, lr=config.g_lr, betas=(config.beta1, config.beta2))
        self.d_optimizer = EngineAdam(self.discriminator, lr=config.d_lr, betas=(config.beta1, config.beta2))
        self.fixed_noise = torch.randn(64, config.latent_dim, device=self.device)
        self.g_losses: List[float] = []
        self.d_losses: List[float] = []
        self.d_real_scores: List[float] = []
        self.d_fake_scores: List[float] = []

    def train_epoch(self) -> Tuple[float, float, float, float]:
        """One pass over the data (ablation_vanilla_gan_signatures.py:397-467): (avg_g_loss, avg_d_loss, avg_d_real,
        avg_d_fake), also appended to the four history lists."""
        self.generator.train()
        self.discriminator.train()
        c = self.config
        epoch_g_loss = epoch_d_loss = epoch_d_real = epoch_d_fake = 0.0
        num_batches = 0
        for real_images in self.data_loader:
            if isinstance(real_images, (list, tuple)):
                real_images = real_images[0]
            real_images = real_images.to(self.device, torch.float32)
            m = self.engine.ablation_step(real_images, lr_d=c.d_lr, lr_g=c.g_lr, beta1=c.beta1, beta2=c.beta2,
                                          label_smoothing=c.label_smoothing)
            epoch_g_loss += m["g_loss"]
            epoch_d_loss += m["d_loss"]
            epoch_d_real += m["d_real_mean"]
            epoch_d_fake += m["d_fake_mean"]
            num_batches += 1
        avg_g_loss = epoch_g_loss / num_batches
        avg_d_loss = epoch_d_loss / num_batches
        avg_d_real = epoch_d_real / num_batches
        avg_d_fake = epoch_d_fake / num_batches
        self.g_losses.append(avg_g_loss)
        self.d_losses.append(avg_d_loss)
        self.d_real_scores.append(avg_d_real)
        self.d_fake_scores.append(avg_d_fake)
        return avg_g_loss, avg_d_loss, avg_d_real, avg_d_fake

    def train(self, progress_bar: bool = False) -> AblationResult:
        """``config.epochs`` epochs, the final sample grid, and the result with its stability metrics (:469-510)."""
        start_time = time.time()
        for epoch in range(1, self.config.epochs + 1):
            g_loss, d_loss, _, _ = self.train_epoch()
            if progress_bar:
                print(f"{self.config.get_short_name()} epoch {epoch}/{self.config.epochs}: G {g_loss:.4f} D {d_loss:.4f}")
        training_time = time.time() - start_time
        sample_path = self._save_samples()
        result = AblationResult(config=self.config, g_losses=self.g_losses, d_losses=self.d_losses,
                                d_real_scores=self.d_real_scores, d_fake_scores=self.d_fake_scores,
                                training_time=training_time, sample_path=str(sample_path))
        result.compute_stability_metrics()
        return result

    def _save_samples(self) -> Path:
        from .train_vanilla_gan_signatures import save_sample_grid
        self.generator.eval()
        with torch.no_grad():
            samples = self.generator(self.fixed_noise)
        sample_path = self.output_dir / "samples" / f"{self.config.get_short_name()}_samples.png"
        sample_path.parent.mkdir(parents=True, exist_ok=True)
        save_sample_grid(samples, sample_path, nrow=8)
        return sample_path

    def generate_samples(self, n_samples: int = 64) -> torch.Tensor:
        """Eval-mode samples (running BatchNorm statistics) from fresh z ~ N(0, 1) of torch's generator (:512-518)."""
        self.generator.eval()
        with torch.no_grad():
            z = torch.randn(n_samples, self.config.latent_dim, device=self.device)
            samples = self.generator(z)
        return samples
