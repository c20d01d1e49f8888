"""Test-side restatement of the ablation study's LeakyReLU Generator (ablation_vanilla_gan_signatures.py:159-328) and of the
iterations that train it, built from the oracle's pieces (oracle.siggan_oracle: _act with a slope, d_forward, bce, AdamState,
sn_weights).  The oracle's own g_forward is the ReLU network; these functions differ from it only in the slope handed to the
Generator's activations.  ``signs`` / ``record`` as in the oracle (see oracle.siggan_oracle._act)."""
import torch
import torch.nn.functional as F

from common import O

SLOPE = 0.2          # ConfigurableGenerator's default leaky_slope, the one AblationGANTrainer uses (ablation...py:361-366)


def g_forward(sd, z, training, size, slope=SLOPE, signs=None, record=None):
    """ConfigurableGenerator.forward (ablation...py:311-328): Linear -> BatchNorm1d -> act, then per block
    ConvTranspose2d -> BatchNorm2d -> act, then 3x3 conv + tanh; act = LeakyReLU(slope) (slope 0: ReLU)."""
    chain = O.G_CHAIN[size]
    sg = (lambda i: None) if signs is None else (lambda i: signs[i])

    def bn(x, prefix):
        if training:
            sd[prefix + "num_batches_tracked"] += 1
        return F.batch_norm(x, sd[prefix + "running_mean"], sd[prefix + "running_var"], sd[prefix + "weight"],
                            sd[prefix + "bias"], training, O.BN_MOMENTUM, O.BN_EPS)

    x = O._act(bn(F.linear(z, sd["fc.0.weight"], sd["fc.0.bias"]), "fc.1."), slope, sg(0), record)
    x = x.view(-1, chain[0], 4, 4)
    for i in range(len(chain) - 1):
        p = f"upsample_blocks.{i}.block."
        x = F.conv_transpose2d(x, sd[p + "0.weight"], None, stride=2, padding=1)
        x = O._act(bn(x, p + "1."), slope, sg(i + 1), record)
    x = F.conv2d(x, sd["final_conv.0.weight"], sd["final_conv.0.bias"], stride=1, padding=1)
    return torch.tanh(x)


def _leafs(sd, names):
    return {k: sd[k].detach().clone().requires_grad_(True) for k in names}


def ablation_step(g_sd, d_sd, g_opt, d_opt, real, z, masks_real, masks_fake, masks_g, size, slope=SLOPE, sn=None,
                  lr_g=2e-4, lr_d=2e-4, beta1=0.5, beta2=0.999, label_smoothing=0.9, dropout=0.25, signs=None, record=None,
                  preds=None):
    """One iteration of AblationGANTrainer.train_epoch (ablation...py:397-467) with the configurable Generator: the statements
    of oracle.ablation_step.  ``sn`` (weight_u / weight_v dict, updated in place): a spectral-norm Discriminator, every
    train-mode pass of which runs one power iteration.  ``signs`` / ``record``: dicts keyed 'g', 'd_real', 'd_fake', 'd_g'.
    ``preds`` (a list, optional) receives the three Discriminator outputs: real, fake.detach(), fake (the G update's)."""
    g_names = O.param_names(O.g_state_specs(z.shape[1], size))
    d_names = O.param_names(O.d_state_specs(size, real.shape[1]))
    g_leaf = dict(g_sd)
    g_leaf.update(_leafs(g_sd, g_names))
    sg = (lambda key: None) if signs is None else (lambda key: signs[key])
    rc = (lambda key: None) if record is None else (lambda key: record.setdefault(key, []))
    w = (lambda d: d) if sn is None else (lambda d: O.sn_weights(d, sn, size, True))
    fake = g_forward(g_leaf, z, True, size, slope, sg("g"), rc("g"))
    for k in g_sd:
        if k not in g_names:
            g_sd[k] = g_leaf[k]
    d_leaf = _leafs(d_sd, d_names)
    real_preds = O.d_forward(w(d_leaf), real, size, masks_real, dropout, signs=sg("d_real"), record=rc("d_real"))
    fake_preds = O.d_forward(w(d_leaf), fake.detach(), size, masks_fake, dropout, signs=sg("d_fake"), record=rc("d_fake"))
    loss_real, loss_fake = O.bce(real_preds, label_smoothing), O.bce(fake_preds, 0.0)
    d_loss = loss_real + loss_fake
    gl = torch.autograd.grad(d_loss, [d_leaf[k] for k in d_names])
    d_grads = {k: g.detach() for k, g in zip(d_names, gl)}
    d_opt.apply(d_sd, d_grads, lr_d, beta1, beta2)
    preds_g = O.d_forward(w(d_sd), fake, size, masks_g, dropout, signs=sg("d_g"), record=rc("d_g"))
    g_loss = O.bce(preds_g, label_smoothing)
    gl = torch.autograd.grad(g_loss, [g_leaf[k] for k in g_names])
    g_grads = {k: g.detach() for k, g in zip(g_names, gl)}
    g_opt.apply(g_sd, g_grads, lr_g, beta1, beta2)
    if preds is not None:
        preds += [p.detach().reshape(-1) for p in (real_preds, fake_preds, preds_g)]
    metrics = {"d_loss": float(d_loss.detach()), "d_loss_real": float(loss_real.detach()), "d_loss_fake": float(loss_fake.detach()),
               "d_real_mean": float(real_preds.detach().mean()), "d_fake_mean": float(fake_preds.detach().mean()),
               "g_loss": float(g_loss.detach()), "g_fake_mean": float(preds_g.detach().mean())}
    return metrics, d_grads, g_grads


def d_step(g_sd, d_sd, d_opt, real, z, masks_real, masks_fake, size, slope=SLOPE, lr=2e-4, beta1=0.5, beta2=0.999,
           label_smoothing=0.9, dropout=0.25, signs=None, record=None):
    """The trainer variant's D step (oracle.d_step) in front of a configurable Generator (eval mode, no gradient).  The
    reference never trains this combination: this pins the engine's arithmetic only."""
    names = O.param_names(O.d_state_specs(size, real.shape[1]))
    leaf = _leafs(d_sd, names)
    with torch.no_grad():
        fake = g_forward(g_sd, z, False, size, slope)
    nb = len(O.D_CHAIN[size])
    s_real, s_fake = (None, None) if signs is None else (signs[:nb], signs[nb:])
    real_preds = O.d_forward(leaf, real, size, masks_real, dropout, signs=s_real, record=record)
    fake_preds = O.d_forward(leaf, fake, size, masks_fake, dropout, signs=s_fake, record=record)
    loss_real, loss_fake = O.bce(real_preds, label_smoothing), O.bce(fake_preds, 0.0)
    loss = loss_real + loss_fake
    gl = torch.autograd.grad(loss, [leaf[k] for k in names])
    grads = {k: g.detach() for k, g in zip(names, gl)}
    d_opt.apply(d_sd, grads, lr, beta1, beta2)
    return {"d_loss": float(loss.detach()), "d_real_mean": float(real_preds.detach().mean()),
            "d_fake_mean": float(fake_preds.detach().mean())}, grads


def g_step(g_sd, d_sd, g_opt, z, size, slope=SLOPE, lr=2e-4, beta1=0.5, beta2=0.999, signs=None, record=None):
    """The trainer variant's G step (oracle.g_step) with a configurable Generator: G train mode, D eval, target 1."""
    names = O.param_names(O.g_state_specs(z.shape[1], size))
    leaf = dict(g_sd)
    leaf.update(_leafs(g_sd, names))
    ng = len(O.G_CHAIN[size])
    s_g, s_d = (None, None) if signs is None else (signs[:ng], signs[ng:])
    fake = g_forward(leaf, z, True, size, slope, s_g, record)
    for k in g_sd:
        if k not in names:
            g_sd[k] = leaf[k]
    preds = O.d_forward(d_sd, fake, size, None, signs=s_d, record=record)
    loss = O.bce(preds, 1.0)
    gl = torch.autograd.grad(loss, [leaf[k] for k in names])
    grads = {k: g.detach() for k, g in zip(names, gl)}
    g_opt.apply(g_sd, grads, lr, beta1, beta2)
    return {"g_loss": float(loss.detach()), "g_fake_mean": float(preds.detach().mean())}, grads
