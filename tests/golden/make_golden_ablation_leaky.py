#!/usr/bin/env python3
"""Fixtures of the ablation study's LeakyReLU Generator, made by running the REFERENCE's own
AblationGANTrainer.train_epoch (ablation_vanilla_gan_signatures.py:397-467) on CPU, fp32:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ablation_leaky.py

That module imports torchvision (absent here) for its data pipeline and plotting only; a stub module
placed in sys.modules first lets it import, and nothing this script runs touches it.  The trainer
builds ConfigurableGenerator(activation="leaky_relu") (:216-328) and the standard Discriminator; their
states and Adam moments are replaced by the synthetic ones of inputs.py, and hooks observe (never
alter) z, the Dropout2d masks and the activation census.  Written: golden_ablation_leaky.npz.

Cases: 64x64 z=200 batch 8; 64x64 z=50 batch 8 with Discriminator(use_spectral_norm=True) (a latent % 4 != 0: the
Generator fc's generic kernels); 128x128 z=128 batch 4.  Per case tag s{S}_z{Z}_b{B}[_sn], in the layout of
golden_ablation_step.npz (make_golden.make_ablation_step):
  <tag>/d/*, <tag>/g/*   the first iteration's metrics, gradient / weight / moment probes (and BatchNorm buffers); the
                         spectral-norm case keys D by the PLAIN parameter names (weight_orig -> weight) in the plain order,
                         and records the weight_u / weight_v buffers after the iteration as <tag>/d/sn/*
  <tag>/preds            D's per-sample outputs of the iteration's three Discriminator calls: real, fake.detach(), fake
  <tag>/census/*         near-zero activation inputs in call order: D(real), G, D(fake.detach()), D(fake) of the G update
  <tag>/masks, <tag>/z   the dropout keep masks (three sets) and the latent batch the trainer drew
  <tag>/eval/z, /img     generate_samples() after that iteration: its z and the eval-mode images
  epoch/*                (first case) a 3-batch train_epoch from the same states: per-iteration z and masks, the four means
"""
import json
import os
import sys
import tempfile
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src")


def _stub(name):
    m = types.ModuleType(name)

    def attr(a):
        if a.startswith("__"):
            raise AttributeError(a)
        return type(a, (), {})
    m.__getattr__ = attr
    sys.modules[name] = m
    return m


_tv = _stub("torchvision")
_tv.transforms, _tv.utils = _stub("torchvision.transforms"), _stub("torchvision.utils")

import numpy as np                                                     # noqa: E402
import torch                                                           # noqa: E402
import torch.nn as nn                                                  # noqa: E402

import inputs as I                                                     # noqa: E402
from make_golden import (SEED_ADAM_D, SEED_ADAM_G, SEED_REAL, SEED_STATE_D, SEED_STATE_G, SEED_TORCH,  # noqa: E402
                         ActTap, MaskTap, load_adam, load_state, probes, record_step)
import ablation_vanilla_gan_signatures as A                           # noqa: E402  (the reference)

CASES = ((64, 200, 8, False), (64, 50, 8, True), (128, 128, 4, False))
EPOCH_BATCHES = 3
EVAL_N = 4


class _LossTap(nn.BCELoss):
    """The trainer's criterion, recording every loss value it returns (d_real, d_fake, g per iteration)."""

    def __init__(self):
        super().__init__()
        self.values = []

    def forward(self, p, y):
        out = super().forward(p, y)
        self.values.append(out.item())
        return out


def _plain(name):
    return name.replace("weight_orig", "weight")


def _trainer(size, latent, batches, sn=False):
    cfg = A.AblationConfig(name="leaky", latent_dim=latent, activation="leaky_relu", use_spectral_norm=sn,
                           image_size=size, batch_size=batches[0].shape[0], epochs=1)
    torch.manual_seed(0)
    t = A.AblationGANTrainer(cfg, batches, torch.device("cpu"), tempfile.gettempdir())
    gs = load_state(t.generator, SEED_STATE_G)
    load_adam(t.g_optimizer, t.generator, gs, SEED_ADAM_G)
    if not sn:
        ds = load_state(t.discriminator, SEED_STATE_D)
        load_adam(t.d_optimizer, t.discriminator, ds, SEED_ADAM_D)
    else:       # as make_golden.make_spectral_norm_steps: weight_orig / u / v from the plain specs, moments by plain name
        plain = A.Discriminator(input_size=size).state_dict()
        plain = {k: (tuple(v.shape), "param") for k, v in plain.items()}
        t.discriminator.load_state_dict({k: torch.from_numpy(v) for k, v in I.gen_sn_state(plain, SEED_STATE_D).items()})
        mm, vv, step = I.gen_adam(plain, SEED_ADAM_D)
        names = [k for k, _ in t.discriminator.named_parameters()]
        sd = t.d_optimizer.state_dict()
        sd["state"] = {i: {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(mm[_plain(k)]).clone(),
                           "exp_avg_sq": torch.from_numpy(vv[_plain(k)]).clone()} for i, k in enumerate(names)}
        t.d_optimizer.load_state_dict(sd)
    t.criterion = _LossTap()
    return t


def _record_d_plain(tag, D, opt, out):
    """record_step for a spectral-norm Discriminator under the plain names and in the plain order (conv weight, bias, ...):
    what the oracle / the engine call these tensors."""
    named = dict(D.named_parameters())
    order = [k for k in A.Discriminator(input_size=D.input_size).state_dict()]
    params = {k: named[k[:-len("weight")] + "weight_orig" if k.endswith(".weight") else k] for k in order}
    out[f"{tag}/grad_norm"] = np.array([float(p.grad.norm()) for p in params.values()], np.float32)
    probes(f"{tag}/grad", {k: p.grad for k, p in params.items()}, out)
    probes(f"{tag}/w", params, out)
    probes(f"{tag}/m", {k: opt.state[p]["exp_avg"] for k, p in params.items()}, out)
    probes(f"{tag}/v", {k: opt.state[p]["exp_avg_sq"] for k, p in params.items()}, out)
    out[f"{tag}/adam_step"] = np.float32(float(opt.state[next(iter(params.values()))]["step"]))


def _z_tap(gen, zs):
    return gen.register_forward_pre_hook(lambda mod, inp: zs.append(inp[0].detach().clone().numpy()))


def first_iteration(size, latent, B, sn, out):
    tag = f"s{size}_z{latent}_b{B}" + ("_sn" if sn else "")
    real = torch.from_numpy(I.gen_real(B, size, SEED_REAL))
    t = _trainer(size, latent, [real], sn)
    G, D = t.generator, t.discriminator
    zs, preds = [], []
    hz = _z_tap(G, zs)
    hp = D.register_forward_hook(lambda mod, inp, o: preds.append(o.detach().reshape(-1).numpy().copy()))
    masks = MaskTap(D)
    acts = ActTap(D, G)                 # appends per CALL: the harness' call order
    d_rec = {}

    def after_d_step(opt, args, kwargs):        # D's gradients before the G update's backward adds to them (:437-446)
        v = t.criterion.values
        d_rec["metrics"] = {"d_loss_real": v[0], "d_loss_fake": v[1]}
        if sn:
            _record_d_plain(f"{tag}/d", D, opt, out)
        else:
            record_step(f"{tag}/d", None, D, opt, {}, out)
    hd = t.d_optimizer.register_step_post_hook(after_d_step)
    torch.manual_seed(SEED_TORCH + 9)
    g_loss, d_loss, d_real, d_fake = t.train_epoch()
    hd.remove(); masks.close(); acts.close(); hz.remove(); hp.remove()
    assert len(preds) == 3
    out[f"{tag}/preds"] = np.stack(preds)
    if sn:
        probes(f"{tag}/d/sn", {k: v for k, v in D.state_dict().items() if k.endswith(("weight_u", "weight_v"))}, out)
    v = t.criterion.values
    assert len(v) == 3 and g_loss == v[2]
    for k, x in dict(d_rec["metrics"], d_loss=d_loss, d_real_mean=d_real, d_fake_mean=d_fake).items():
        out[f"{tag}/d/metric/{k}"] = np.float32(x)
    acts.store(tag, out)
    record_step(f"{tag}/g", None, G, t.g_optimizer, {"g_loss": g_loss}, out, extra_buffers=True)
    nb = 4 if size == 64 else 5
    assert len(masks.masks) == 3 * nb and len(zs) == 1
    out[f"{tag}/masks"] = I.pack_masks(masks.masks)
    out[f"{tag}/z"] = zs[0]
    # generate_samples after the iteration: eval mode, running statistics (:512-518)
    zs.clear()
    hz = _z_tap(G, zs)
    torch.manual_seed(SEED_TORCH + 10)
    img = t.generate_samples(EVAL_N)
    hz.remove()
    out[f"{tag}/eval/z"] = zs[0]
    out[f"{tag}/eval/img"] = img.numpy()


def epoch_means(size, latent, B, out):
    batches = [torch.from_numpy(I.gen_real(B, size, SEED_REAL + k)) for k in range(EPOCH_BATCHES)]
    t = _trainer(size, latent, batches)
    zs = []
    hz = _z_tap(t.generator, zs)
    masks = MaskTap(t.discriminator)
    torch.manual_seed(SEED_TORCH + 11)
    means = t.train_epoch()
    hz.remove(); masks.close()
    assert len(zs) == EPOCH_BATCHES
    out["epoch/case"] = np.array([size, latent, B, EPOCH_BATCHES], np.int32)
    out["epoch/z"] = np.stack(zs)
    out["epoch/masks"] = I.pack_masks(masks.masks)
    out["epoch/means"] = np.array(means, np.float32)                  # avg_g_loss, avg_d_loss, avg_d_real, avg_d_fake
    out["epoch/lists"] = np.array([t.g_losses, t.d_losses, t.d_real_scores, t.d_fake_scores], np.float32)


def main():
    torch.set_num_threads(8)
    out = {}
    for size, latent, B, sn in CASES:
        first_iteration(size, latent, B, sn, out)
    epoch_means(*CASES[0][:3], out)
    keys = {f"s{s}_z{z}": list(A.ConfigurableGenerator(latent_dim=z, output_size=s, activation="leaky_relu").state_dict())
            for s, z, _, _ in CASES}
    out["meta"] = np.array(json.dumps({"torch": torch.__version__, "threads": torch.get_num_threads(), "label_smoothing": 0.9,
                                       "leaky_slope": 0.2, "g_state_dict_keys": keys,
                                       "seeds": dict(real=SEED_REAL, torch=SEED_TORCH + 9, eval=SEED_TORCH + 10,
                                                     epoch=SEED_TORCH + 11)}))
    path = os.path.join(HERE, "golden_ablation_leaky.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
