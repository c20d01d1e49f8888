"""Signature verification model training on the MI355X HIP path.

Drop-in for the reference's ``signature_verifier_train`` module: the Siamese CNN with the reference's constructors and
``state_dict()`` keys, its pair dataset (same ``random`` draws, so the same seed gives the same pairs), ``train_epoch`` /
``evaluate`` / ``train_model`` / ``main`` with the reference's signatures, printed lines, 80/20 split, checkpoint
dictionaries and file names.  One batch is ONE fused train step in HIP (include/siggan_verifier_train.h,
csrc/verifier_train.hip): train-mode forward, BCE + contrastive loss, backward and Adam; eval-mode forwards go through the
eval module's context (include/siggan_verifier.h).  There is no PyTorch fallback.

The parameters of a model that has trained are views into one flat arena (gradients and Adam moments likewise); metrics
are accumulated on the device and read once per epoch.

The reference's random training transforms (RandomAffine, RandomHorizontalFlip) run on the CPU through torchvision when it
can be imported; without it ``train_model`` trains on the deterministic chain and says so in one line.  That is the default
``input_pipeline="host"``.  With ``input_pipeline="device"`` (``--input_pipeline device``) the images are decoded once into an
HBM-resident uint8 cache and every batch is gathered and augmented by one HIP launch with the reference's draws
(``verifier_data.DevicePairLoader``); torchvision is not needed.

Beyond the reference, and off by default: ``hard_mining`` (``--hard_mining K``, device pipeline only) adds to every epoch from
``hard_mining_start`` on the pairs the current weights get most wrong -- per signature its K highest-scoring impostors and its
lowest-scoring genuine partners, taken from one all-pairs pass in HIP (``verifier_mining``).  ``elastic`` (``--elastic PX``, device
pipeline only) sends every augmented training batch through one more HIP launch, the smooth random warp of ``warp.warp_u8`` with
control displacements of up to PX pixels: genuine-looking variation the rigid RandomAffine cannot give.  Whether it improves
accuracy is not measured.
"""
import argparse
import ctypes as C
import random
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from PIL import Image
from torch.utils.data import DataLoader, Dataset

from . import _lib
from . import signature_verifier_eval as SV
from .signature_verifier_eval import CNNEncoder, _ptr            # noqa: F401  (CNNEncoder: the reference's name)

DEFAULT_MAX_PAIRS = 32
METRICS = ("loss", "bce_loss", "contrastive_loss", "n_correct")


class _Trainer:
    """One siggan_verifier_trainer handle bound to the model's arenas and running tensors."""

    def __init__(self, device, embedding_dim, max_pairs):
        self.lib = _lib.load()
        self.device, self.E, self.max_pairs = device, int(embedding_dim), int(max_pairs)
        h = C.c_void_p()
        _lib.check(self.lib.siggan_verifier_trainer_create(device.index, self.E, self.max_pairs, C.byref(h)))
        self._h = h
        self.count = int(self.lib.siggan_verifier_trainer_param_count(h))
        self.spans = []
        for i in range(_lib.VT_PARAM_TENSORS):
            off, n = C.c_int64(), C.c_int64()
            _lib.check(self.lib.siggan_verifier_trainer_param_span(h, i, C.byref(off), C.byref(n)))
            self.spans.append((off.value, n.value))

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def bind(self, arenas, running, bn_eps, adam_step):
        st = _lib.VerifierTrainStorage()
        for name, t in zip(("params", "grads", "exp_avg", "exp_avg_sq"), arenas):
            setattr(st, name, t.data_ptr())
        for name, t in zip(_lib.VT_RUNNING_FIELDS, running):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous float32 tensor on {self.device}")
            setattr(st, name, t.data_ptr())
        st.bn_eps = float(bn_eps)
        self._keep = (arenas, running)
        _lib.check(self.lib.siggan_verifier_trainer_bind(self._h, C.byref(st), int(adam_step)))

    def seed(self, seed, offset=0):
        _lib.check(self.lib.siggan_verifier_trainer_seed(self._h, int(seed), int(offset)))

    def debug(self, name, shape, dtype=torch.uint8):
        n = 1
        for s in shape:
            n *= int(s)
        out = torch.empty(n, dtype=dtype, device=self.device)
        _lib.check(self.lib.siggan_verifier_train_debug(self._h, name.encode(), _ptr(out), n, self.stream()))
        return out.view(*shape)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.siggan_verifier_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                                   # interpreter shutdown
            pass


class SiameseNetwork(SV.SiameseNetwork):
    """The reference's SiameseNetwork.  ``.eval()`` forwards are the eval module's; in training mode a batch goes through
    ``train_step`` (``train_epoch`` calls it) -- a train-mode ``forward`` has no autograd graph to hand out and raises."""

    def __init__(self, embedding_dim: int = 128, max_images: int = SV.DEFAULT_MAX_IMAGES, max_pairs: int = DEFAULT_MAX_PAIRS) -> None:
        super().__init__(embedding_dim=embedding_dim, max_images=max_images)
        self.max_pairs = int(max_pairs)
        self._trainer = None
        self._arenas = None
        self._adam_step = 0
        self._seed = None

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._drop_trainer()
        return out

    def _drop_trainer(self):
        if getattr(self, "_trainer", None) is not None:
            self._trainer.close()
        self._trainer, self._arenas = None, None

    def seed_dropout(self, seed: int, offset: int = 0):
        """Seed of the library's counter-based RNG that draws the dropout keep masks."""
        self._seed = (int(seed), int(offset))
        if self._trainer is not None:
            self._trainer.seed(*self._seed)

    def _running(self):
        enc = self.encoder
        return [t for bn in (enc.bn1, enc.bn2, enc.bn3) for t in (bn.running_mean, bn.running_var)]

    def trainer(self, n_pairs: int = 1) -> _Trainer:
        """The train context (created on first use; parameters become views into its arena)."""
        params = list(self.parameters())
        dev = params[0].device
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} {SV._NO_CPU}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._trainer is not None and n_pairs <= self._trainer.max_pairs:
            return self._trainer
        if self._trainer is not None:
            self._trainer.close()
        t = _Trainer(dev, self.embedding_dim, max(self.max_pairs, int(n_pairs)))
        if self._arenas is None:
            arenas = [torch.zeros(t.count, dtype=torch.float32, device=dev) for _ in range(4)]
            with torch.no_grad():
                for p, (off, n) in zip(params, t.spans):
                    if p.numel() != n or p.dtype != torch.float32:
                        raise ValueError("the model's parameters do not match the library's arena")
                    arenas[0][off:off + n].copy_(p.reshape(-1))
                    p.data = arenas[0][off:off + n].view(p.shape)
                    p.grad = arenas[1][off:off + n].view(p.shape)
            self._arenas = arenas
        eps = self.encoder.bn1.eps
        t.bind(self._arenas, self._running(), eps, self._adam_step)
        if self._seed is not None:
            t.seed(*self._seed)
        self._trainer = t
        return t

    def arena_views(self, which: str) -> "Dict[str, torch.Tensor]":
        """name -> view for which in 'params' | 'grads' | 'exp_avg' | 'exp_avg_sq'."""
        t = self.trainer()
        a = self._arenas[("params", "grads", "exp_avg", "exp_avg_sq").index(which)]
        return {n: a[off:off + cnt].view(p.shape) for (n, p), (off, cnt) in zip(self.named_parameters(), t.spans)}

    def _batch(self, x1, x2, labels, fc_keep, cls_keep):
        if not self.training:
            raise RuntimeError(f"{type(self).__name__}: train_step / compute_grads need training mode (call .train())")
        t = self.trainer(x1.shape[0])
        ctx_images = SV._Context._images
        x1, fmt, n = ctx_images(t, x1, "x1")
        x2, fmt2, n2 = ctx_images(t, x2, "x2")
        if fmt != fmt2 or n != n2:
            raise ValueError("x1 and x2 must have the same dtype and batch size")
        labels = labels.to(device=t.device, dtype=torch.float32).reshape(-1).contiguous()
        if labels.numel() != n:
            raise ValueError(f"labels must hold {n} values, got {labels.numel()}")
        masks = []
        for m, shape, what in ((fc_keep, (2 * n, 512), "fc_keep"), (cls_keep, (n, 64), "cls_keep")):
            if m is not None:
                if tuple(m.shape) != shape or m.dtype != torch.float32 or m.device != t.device:
                    raise ValueError(f"{what} must be float32 {shape} on {t.device}")
                m = m.contiguous()
            masks.append(m)
        return t, x1, x2, fmt, n, labels, masks

    def _stepped(self):
        with torch.no_grad():
            for bn in (self.encoder.bn1, self.encoder.bn2, self.encoder.bn3):
                bn.num_batches_tracked += 2                  # the encoder ran twice
        self.params_changed()                                # the eval context's packs / folded tables are stale

    def compute_grads(self, x1, x2, labels, use_contrastive=True, fc_keep=None, cls_keep=None):
        """Train-mode forward + losses + backward: fills the gradient arena (``p.grad``), updates the running statistics;
        returns the device tensor (loss, bce, contrastive, n_correct)."""
        t, x1, x2, fmt, n, labels, (fk, ck) = self._batch(x1, x2, labels, fc_keep, cls_keep)
        metrics = torch.empty(_lib.VT_METRICS, dtype=torch.float32, device=t.device)
        _lib.check(t.lib.siggan_verifier_train_grads(t._h, _ptr(x1), _ptr(x2), fmt, _ptr(labels), n, _ptr(fk), _ptr(ck),
                                                     1 if use_contrastive else 0, _ptr(metrics), t.stream()))
        self._stepped()
        return metrics

    def apply_grads(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        t = self.trainer()
        _lib.check(t.lib.siggan_verifier_train_apply(t._h, float(lr), float(beta1), float(beta2), float(eps), t.stream()))
        self._adam_step += 1
        self.params_changed()

    def train_step(self, x1, x2, labels, optimizer, use_contrastive=True, fc_keep=None, cls_keep=None):
        """One fused step (gradients + the optimiser's Adam update, its ``lr`` read now); returns the device tensor
        (loss, bce, contrastive, n_correct)."""
        t, x1, x2, fmt, n, labels, (fk, ck) = self._batch(x1, x2, labels, fc_keep, cls_keep)
        h = optimizer.hyper()
        metrics = torch.empty(_lib.VT_METRICS, dtype=torch.float32, device=t.device)
        _lib.check(t.lib.siggan_verifier_train_step(t._h, _ptr(x1), _ptr(x2), fmt, _ptr(labels), n, _ptr(fk), _ptr(ck),
                                                    1 if use_contrastive else 0, h["lr"], h["beta1"], h["beta2"], h["eps"],
                                                    _ptr(metrics), t.stream()))
        self._adam_step += 1
        optimizer._opt_called = True                         # an lr_scheduler on it sees that the optimiser has stepped
        self._stepped()
        return metrics


class Adam(torch.optim.Adam):
    """torch.optim.Adam over a SiameseNetwork whose ``step`` is the HIP update; ``lr`` is read at every step, so
    torch.optim.lr_scheduler.StepLR works on it, and ``state_dict()`` loads into a plain torch.optim.Adam."""

    def __init__(self, model: SiameseNetwork, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        if not isinstance(model, SiameseNetwork):
            raise TypeError("Adam(model, ...) takes the SiameseNetwork of this module, not its parameters()")
        super().__init__(list(model.parameters()), lr=lr, betas=betas, eps=eps)
        self._model = model

    def hyper(self):
        g = self.param_groups[0]
        return dict(lr=float(g["lr"]), beta1=float(g["betas"][0]), beta2=float(g["betas"][1]), eps=float(g["eps"]))

    def _sync(self):
        m = self._model
        if m._adam_step == 0 and not self.state:
            return
        ea, es = m.arena_views("exp_avg"), m.arena_views("exp_avg_sq")
        for n, p in m.named_parameters():
            self.state[p] = {"step": torch.tensor(float(m._adam_step)), "exp_avg": ea[n], "exp_avg_sq": es[n]}

    def state_dict(self):
        self._sync()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        m = self._model
        for g, new in zip(self.param_groups, state_dict["param_groups"]):
            g.update({k: v for k, v in new.items() if k != "params"})
        ea, es = m.arena_views("exp_avg"), m.arena_views("exp_avg_sq")
        names = [n for n, _ in m.named_parameters()]
        step = 0
        with torch.no_grad():
            for idx, st in state_dict["state"].items():
                ea[names[int(idx)]].copy_(st["exp_avg"]); es[names[int(idx)]].copy_(st["exp_avg_sq"])
                step = int(float(st["step"]))
        m._adam_step = step
        t = m.trainer()
        t.bind(m._arenas, m._running(), m.encoder.bn1.eps, step)
        self._sync()

    def zero_grad(self, set_to_none=True):
        pass                                                 # every compute_grads / train_step writes the whole gradient arena

    @torch.no_grad()
    def step(self, closure=None):
        """Apply the HIP Adam update to the gradients of the last ``compute_grads``."""
        self._model.apply_grads(**self.hyper())


class ContrastiveLoss(nn.Module):
    """mean(Y * D^2 + (1 - Y) * clamp(margin - D, 0)^2), Y = 1 for a same-writer pair, D = F.pairwise_distance.  The train
    step computes this term in HIP; the module is here for callers that want the value of a batch of embeddings."""

    def __init__(self, margin: float = 2.0) -> None:
        super().__init__()
        self.margin = margin

    def forward(self, embedding1: torch.Tensor, embedding2: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        d = F.pairwise_distance(embedding1, embedding2)
        return (label * d.pow(2) + (1 - label) * torch.clamp(self.margin - d, min=0.0).pow(2)).mean()


class SignaturePairDataset(Dataset):
    """Genuine-genuine pairs (label 1) and genuine-other pairs (label 0) with the reference's directory rules and its
    ``random`` draws in the reference's order."""

    def __init__(self, data_dir: str, synthetic_dir: Optional[str] = None, transform=None, pairs_per_user: int = 10) -> None:
        self.data_dir = Path(data_dir)
        self.synthetic_dir = Path(synthetic_dir) if synthetic_dir else None
        self.pairs_per_user = pairs_per_user
        self.transform = transform or SV.default_transform
        self.user_signatures: Dict[str, List[Path]] = {}
        self._load_signatures()
        self.pairs: List[Tuple[Path, Path, int]] = []
        self._generate_pairs()

    def _load_signatures(self) -> None:
        image_extensions = {'.png', '.jpg', '.jpeg', '.bmp', '.tiff'}
        subdirs = [d for d in self.data_dir.iterdir() if d.is_dir()]
        if subdirs:
            for user_dir in subdirs:
                user_images = [f for f in user_dir.iterdir() if f.suffix.lower() in image_extensions]
                if len(user_images) >= 2:
                    self.user_signatures[user_dir.name] = user_images
        else:
            for img_path in [f for f in self.data_dir.iterdir() if f.suffix.lower() in image_extensions]:
                parts = img_path.stem.split('_')
                user_id = parts[0] if parts else img_path.stem
                self.user_signatures.setdefault(user_id, []).append(img_path)
            self.user_signatures = {k: v for k, v in self.user_signatures.items() if len(v) >= 2}
        if self.synthetic_dir and self.synthetic_dir.exists():
            synthetic_images = [f for f in self.synthetic_dir.iterdir() if f.suffix.lower() in image_extensions]
            if synthetic_images:
                self.user_signatures['_synthetic_'] = synthetic_images
        print(f"Loaded {len(self.user_signatures)} users with signatures")
        for user_id, sigs in self.user_signatures.items():
            print(f"  {user_id}: {len(sigs)} signatures")

    def _generate_pairs(self) -> None:
        user_ids = list(self.user_signatures.keys())
        for user_id in user_ids:
            user_sigs = self.user_signatures[user_id]
            if user_id == '_synthetic_':
                continue
            for _ in range(self.pairs_per_user):
                if len(user_sigs) >= 2:
                    sig1, sig2 = random.sample(user_sigs, 2)
                    self.pairs.append((sig1, sig2, 1))
            other_users = [u for u in user_ids if u != user_id]
            for _ in range(self.pairs_per_user):
                if other_users:
                    other_user = random.choice(other_users)
                    sig1 = random.choice(user_sigs)
                    sig2 = random.choice(self.user_signatures[other_user])
                    self.pairs.append((sig1, sig2, 0))
        random.shuffle(self.pairs)
        print(f"Generated {len(self.pairs)} pairs")

    def __len__(self) -> int:
        return len(self.pairs)

    def __getitem__(self, idx: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        sig1_path, sig2_path, label = self.pairs[idx]
        img1 = Image.open(sig1_path).convert('L')
        img2 = Image.open(sig2_path).convert('L')
        if self.transform:
            img1 = self.transform(img1)
            img2 = self.transform(img2)
        return img1, img2, torch.tensor(label, dtype=torch.float32)


def train_epoch(model: SiameseNetwork, dataloader: DataLoader, optimizer: Adam, criterion_bce=None, criterion_contrastive=None,
                device: Optional[torch.device] = None, use_contrastive: bool = True) -> Dict[str, float]:
    """One epoch, one fused HIP train step per batch.  The two criterion arguments are accepted for the reference's
    signature; the losses are the train step's own (BCELoss, ContrastiveLoss(margin=2.0))."""
    model.train()
    device = torch.device(device) if device is not None else next(model.parameters()).device
    acc, total, num_batches = None, 0, 0
    for img1, img2, labels in dataloader:
        m = model.train_step(img1.to(device), img2.to(device), labels.to(device), optimizer, use_contrastive=use_contrastive)
        acc = m.clone() if acc is None else acc + m
        total += labels.size(0)
        num_batches += 1
    loss, bce, con, correct = acc.tolist() if acc is not None else (0.0, 0.0, 0.0, 0.0)      # the epoch's one device read
    nb = max(num_batches, 1)
    return {'loss': loss / nb, 'bce_loss': bce / nb, 'contrastive_loss': con / nb if use_contrastive else 0.0,
            'accuracy': correct / total if total > 0 else 0.0}


def evaluate(model: SiameseNetwork, dataloader: DataLoader, criterion_bce=None, device: Optional[torch.device] = None) -> Dict[str, float]:
    """Eval-mode forwards through the HIP eval context; loss and accuracy accumulated on the device."""
    model.eval()
    device = torch.device(device) if device is not None else next(model.parameters()).device
    criterion_bce = criterion_bce or nn.BCELoss()
    acc, total, num_batches = torch.zeros(2, device=device), 0, 0
    with torch.no_grad():
        for img1, img2, labels in dataloader:
            labels = labels.to(device)
            _, _, similarity = model(img1.to(device), img2.to(device))
            s = similarity.reshape(-1)
            acc[0] += criterion_bce(s, labels)
            acc[1] += ((s > 0.5).float() == labels).sum()
            total += labels.size(0)
            num_batches += 1
    loss, correct = acc.tolist()
    return {'loss': loss / max(num_batches, 1), 'accuracy': correct / total if total > 0 else 0.0}


def _transforms():
    """(train_transform, eval_transform): the reference's chains through torchvision when it imports."""
    try:
        from torchvision import transforms
    except ImportError:
        print("torchvision is not available: training without RandomAffine / RandomHorizontalFlip augmentation")
        return SV.default_transform, SV.default_transform
    train = transforms.Compose([
        transforms.Resize((64, 64)), transforms.Grayscale(num_output_channels=1),
        transforms.RandomAffine(degrees=5, translate=(0.1, 0.1), scale=(0.9, 1.1)), transforms.RandomHorizontalFlip(p=0.1),
        transforms.ToTensor(), transforms.Normalize(mean=[0.5], std=[0.5])])
    return train, SV.default_transform


INPUT_PIPELINES = ("host", "device")
MINING_FLAGS = ("hard_mining", "hard_mining_genuine", "hard_mining_start", "hard_mining_every")


def check_hard_mining(input_pipeline, hard_mining, hard_mining_genuine=None, hard_mining_start=2, hard_mining_every=1):
    """None when mining is off, else the checked (k_impostor, k_genuine, first epoch (1-based), period in epochs)."""
    if hard_mining is None:
        if hard_mining_genuine is not None:
            raise ValueError("hard_mining_genuine needs hard_mining")
        return None
    if input_pipeline != "device":
        raise ValueError("hard mining needs --input_pipeline device (the signatures are mined from the device loader's cache); "
                         f"got input_pipeline={input_pipeline!r}")
    k_imp = int(hard_mining)
    k_gen = k_imp if hard_mining_genuine is None else int(hard_mining_genuine)
    if not 1 <= k_imp <= _lib.PAIR_TOPK_MAX or not 0 <= k_gen <= _lib.PAIR_TOPK_MAX:
        raise ValueError(f"hard_mining must be in 1 .. {_lib.PAIR_TOPK_MAX} and hard_mining_genuine in 0 .. {_lib.PAIR_TOPK_MAX}, "
                         f"got {hard_mining} and {hard_mining_genuine}")
    start, every = int(hard_mining_start), int(hard_mining_every)
    if start < 1 or every < 1:
        raise ValueError(f"hard_mining_start and hard_mining_every must be >= 1, got {hard_mining_start} and {hard_mining_every}")
    return k_imp, k_gen, start, every


ELASTIC_FLAGS = ("elastic", "elastic_cell")


def check_elastic(input_pipeline, elastic, elastic_cell=None):
    """None when the elastic warp is off, else the checked warp.WarpSpec: amplitude ``elastic`` pixels on both axes, control
    cell ``elastic_cell`` (default 16), no affine part (RandomAffine has run already)."""
    if elastic is None:
        if elastic_cell is not None:
            raise ValueError("elastic_cell needs elastic")
        return None
    if input_pipeline != "device":
        raise ValueError("the elastic warp needs --input_pipeline device (it runs on the device loader's batches); "
                         f"got input_pipeline={input_pipeline!r}")
    from .warp import WarpSpec
    return WarpSpec(cell=16 if elastic_cell is None else elastic_cell, amplitude=(elastic, elastic)).check()


def _fit(tag: str, dataset, epochs, output_path, file_name, batch_size, learning_rate, embedding_dim, device, extra,
         input_pipeline: str = "host", mining=None, elastic=None):
    train_size = int(0.8 * len(dataset))
    val_size = len(dataset) - train_size
    train_dataset, val_dataset = torch.utils.data.random_split(dataset, [train_size, val_size])
    if input_pipeline == "device":
        from .verifier_data import DevicePairLoader
        if mining is not None:
            from .verifier_mining import MiningPairLoader
            train_loader = MiningPairLoader(train_dataset, batch_size, shuffle=True, augment=True, k_impostor=mining[0],
                                            k_genuine=mining[1], exclude_dataset=val_dataset, device=device, elastic=elastic)
        else:
            train_loader = DevicePairLoader(train_dataset, batch_size, shuffle=True, augment=True, device=device, elastic=elastic)
        val_loader = DevicePairLoader(val_dataset, batch_size, shuffle=False, augment=False, device=device)
    else:
        train_loader = DataLoader(train_dataset, batch_size=batch_size, shuffle=True, num_workers=0)
        val_loader = DataLoader(val_dataset, batch_size=batch_size, shuffle=False, num_workers=0)
    model = SiameseNetwork(embedding_dim=embedding_dim, max_pairs=batch_size).to(device)
    optimizer = Adam(model, lr=learning_rate)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=10, gamma=0.5)
    criterion_bce = nn.BCELoss()
    best_val_acc = 0.0
    path = output_path / file_name
    for epoch in range(epochs):
        if mining is not None and epoch + 1 >= mining[2] and (epoch + 1 - mining[2]) % mining[3] == 0:
            print("  -> Mined %d hard pairs (%d impostor, %d genuine)" % train_loader.remine(model))
        train_metrics = train_epoch(model, train_loader, optimizer, criterion_bce, None, device)
        val_metrics = evaluate(model, val_loader, criterion_bce, device)
        scheduler.step()
        print(f"Epoch [{epoch+1}/{epochs}] "
              f"Train Loss: {train_metrics['loss']:.4f}, "
              f"Train Acc: {train_metrics['accuracy']:.4f}, "
              f"Val Loss: {val_metrics['loss']:.4f}, "
              f"Val Acc: {val_metrics['accuracy']:.4f}")
        if val_metrics['accuracy'] > best_val_acc:
            best_val_acc = val_metrics['accuracy']
            torch.save(checkpoint_dict(model, embedding_dim, best_val_acc, epoch + 1, **extra), path)
            print(f"  -> Saved best {tag} model (val_acc: {best_val_acc:.4f})")
    return path


def checkpoint_dict(model, embedding_dim, val_accuracy, epoch, **extra):
    """The reference's checkpoint dictionary (tensors detached from the arena)."""
    return {'model_state_dict': {k: v.detach().clone() for k, v in model.state_dict().items()}, 'embedding_dim': embedding_dim,
            'val_accuracy': val_accuracy, 'epoch': epoch, **extra}


def train_model(data_dir: str, synthetic_dir: Optional[str], epochs: int, model_output: str, batch_size: int = 32,
                learning_rate: float = 0.001, embedding_dim: int = 128, device: Optional[str] = None,
                input_pipeline: str = "host", hard_mining: Optional[int] = None, hard_mining_genuine: Optional[int] = None,
                hard_mining_start: int = 2, hard_mining_every: int = 1, elastic: Optional[float] = None,
                elastic_cell: Optional[int] = None) -> Dict[str, str]:
    """Trains the baseline model (real signatures) and, with a synthetic directory, the augmented one (real + synthetic);
    returns the paths of the saved best-validation checkpoints.  input_pipeline: "host" (the reference's DataLoader over
    Pillow decodes) or "device" (HBM-resident cache + one augmentation launch per batch; module docstring).
    hard_mining: K (1 .. 16) turns hard-pair mining on (device pipeline only): from epoch ``hard_mining_start`` (1-based) on,
    every ``hard_mining_every`` epochs, each real signature's K highest-scoring impostors and ``hard_mining_genuine`` (default K)
    lowest-scoring genuine partners under the current weights join the epoch's pairs; the validation split's pairs are never
    mined.
    elastic: PX turns the elastic warp of the training batches on (device pipeline only): control displacements of up to PX
    pixels per axis (at most 0.4 * ``elastic_cell``; cell 8, 16 or 32, default 16) after the reference's augmentation."""
    if input_pipeline not in INPUT_PIPELINES:
        raise ValueError(f"input_pipeline must be one of {INPUT_PIPELINES}, got {input_pipeline!r}")
    mining = check_hard_mining(input_pipeline, hard_mining, hard_mining_genuine, hard_mining_start, hard_mining_every)
    elastic = check_elastic(input_pipeline, elastic, elastic_cell)
    if device is None:
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"train_model: the verifier {SV._NO_CPU}")
    print(f"Training on device: {device}")
    output_path = Path(model_output)
    output_path.mkdir(parents=True, exist_ok=True)
    train_transform = None if input_pipeline == "device" else _transforms()[0]      # the device loader decodes the files itself
    saved_models = {}

    print("\n" + "="*60)
    print("Training BASELINE model (real signatures only)")
    print("="*60)
    baseline_dataset = SignaturePairDataset(data_dir=data_dir, synthetic_dir=None, transform=train_transform, pairs_per_user=20)
    if len(baseline_dataset) == 0:
        print("WARNING: No training pairs generated for baseline model.")
        print("Please ensure data directory contains signature images organized by user.")
    else:
        baseline_path = _fit("baseline", baseline_dataset, epochs, output_path, 'baseline_siamese_model.pth', batch_size,
                             learning_rate, embedding_dim, device, {}, input_pipeline, mining, elastic)
        saved_models['baseline'] = str(baseline_path)
        print(f"\nBaseline model saved to: {baseline_path}")

    if synthetic_dir and Path(synthetic_dir).exists():
        print("\n" + "="*60)
        print("Training AUGMENTED model (real + synthetic signatures)")
        print("="*60)
        augmented_dataset = SignaturePairDataset(data_dir=data_dir, synthetic_dir=synthetic_dir, transform=train_transform,
                                                 pairs_per_user=20)
        if len(augmented_dataset) == 0:
            print("WARNING: No training pairs generated for augmented model.")
        else:
            augmented_path = _fit("augmented", augmented_dataset, epochs, output_path, 'augmented_siamese_model.pth', batch_size,
                                  learning_rate, embedding_dim, device, {'includes_synthetic': True}, input_pipeline, mining, elastic)
            saved_models['augmented'] = str(augmented_path)
            print(f"\nAugmented model saved to: {augmented_path}")
    else:
        print("\nNo synthetic directory provided or directory doesn't exist.")
        print("Skipping augmented model training.")
    return saved_models


def main(argv=None):
    parser = argparse.ArgumentParser(description='Train Siamese network for signature verification',
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('--data_dir', type=str, required=True, help='Directory containing real signature images (organized by user)')
    parser.add_argument('--synthetic_dir', type=str, default=None, help='Optional directory containing synthetic/GAN-generated signatures')
    parser.add_argument('--epochs', type=int, default=50, help='Number of training epochs')
    parser.add_argument('--model_output', type=str, default='./models', help='Output directory for saved models')
    parser.add_argument('--batch_size', type=int, default=32, help='Training batch size')
    parser.add_argument('--learning_rate', type=float, default=0.001, help='Learning rate for optimizer')
    parser.add_argument('--embedding_dim', type=int, default=128, help='Dimension of embedding vectors')
    parser.add_argument('--device', type=str, default=None, choices=['cuda', 'cpu'], help='Device to train on (default: auto-detect)')
    parser.add_argument('--input_pipeline', type=str, default='host', choices=list(INPUT_PIPELINES),
                        help='host: DataLoader over Pillow decodes; device: HBM-resident cache + on-device augmentation')
    # (the mining flags appear in the namespace only when given, so the namespace of a command line without them is what it
    #  was before they existed; train_model holds their defaults)
    later = dict(type=int, default=argparse.SUPPRESS)
    parser.add_argument('--hard_mining', metavar='K', **later,
                        help='Hard-pair mining (needs --input_pipeline device): add each signature\'s K highest-scoring impostors '
                             'under the current weights to the epoch\'s pairs (1 .. 16; default: off)')
    parser.add_argument('--hard_mining_genuine', metavar='K', **later,
                        help='With --hard_mining: lowest-scoring genuine partners per signature (default: the value of --hard_mining)')
    parser.add_argument('--hard_mining_start', metavar='E', **later,
                        help='With --hard_mining: first epoch, 1-based, that trains on mined pairs (default: 2)')
    parser.add_argument('--hard_mining_every', metavar='N', **later, help='With --hard_mining: mine again every N epochs (default: 1)')
    parser.add_argument('--elastic', metavar='PX', type=float, default=argparse.SUPPRESS,
                        help='Elastic warp of the training batches (needs --input_pipeline device): smooth random control '
                             'displacements of up to PX pixels per axis, at most 0.4 cells (default: off)')
    parser.add_argument('--elastic_cell', metavar='C', **later, help='With --elastic: pixels between control points, 8, 16 or 32 (default: 16)')
    args = parser.parse_args(argv)
    mining = {k: getattr(args, k) for k in MINING_FLAGS + ELASTIC_FLAGS if hasattr(args, k)}

    print("="*60)
    print("Signature Verification Model Training")
    print("="*60)
    print(f"Data directory: {args.data_dir}")
    print(f"Synthetic directory: {args.synthetic_dir}")
    print(f"Epochs: {args.epochs}")
    print(f"Batch size: {args.batch_size}")
    print(f"Learning rate: {args.learning_rate}")
    print(f"Embedding dimension: {args.embedding_dim}")
    print(f"Model output: {args.model_output}")
    print("="*60)

    saved_models = train_model(data_dir=args.data_dir, synthetic_dir=args.synthetic_dir, epochs=args.epochs,
                               model_output=args.model_output, batch_size=args.batch_size, learning_rate=args.learning_rate,
                               embedding_dim=args.embedding_dim, device=args.device, input_pipeline=args.input_pipeline, **mining)

    print("\n" + "="*60)
    print("Training Complete!")
    print("="*60)
    print("Saved models:")
    for model_name, model_path in saved_models.items():
        print(f"  - {model_name}: {model_path}")
    return saved_models


if __name__ == '__main__':
    main()
