"""Fixtures of the signature verifier's TRAIN step, made by running the REFERENCE's own SiameseNetwork, ContrastiveLoss,
backward() and torch.optim.Adam.step() (signature_verifier_train.py:376-449) on the CPU, in fp32 and in fp64.  Run once where
the reference is checked out; the outputs are committed:

    python tests/golden/make_golden_verifier_train.py

Nothing of the reference is copied: its module is imported at run time, fed the synthetic state, images, labels and keep
masks of verifier_inputs.py / verifier_train_inputs.py, and only its OUTPUTS are stored.  The three Dropout modules are
replaced by multipliers with the fixed keep masks (mask / (1 - p)).

golden_verifier_train_p<pairs>_e<E>.npz, keys "<variant>s<step>_<name>[_f32|_f64]" (variant "" or "nc_" = use_contrastive 0):
  loss / bce / contrastive / n_correct, e1, e2, similarity, distance
  grad:<param>, param:<param>, exp_avg:<param>, exp_avg_sq:<param> after the step -- tensors up to 4096 elements in full,
      larger ones at verifier_train_inputs.stored_idx positions -- and the six running tensors
  from the fp64 run only: route1 / route2 / route3 (uint8, NCHW, 0..3 = first maximal window element in (dy, dx) order, 4 = max
      not positive), fc1_mask, cls_mask (variant "" only: the forward is the same), and tie:<decision> = flat positions of the decisions whose fp64 margin (winner to
      runner-up or to zero, relative to the layer's max-abs) is below 1e-5
"""
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/src")

import numpy as np                                                    # noqa: E402
import torch                                                          # noqa: E402

# the reference module imports torchvision and PIL at the top (its dataset and train_model use them); empty stand-ins are
# enough for the model, the loss and the optimiser step
if "torchvision" not in sys.modules:
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Compose = object
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms

import verifier_inputs as VI                                          # noqa: E402
import verifier_train_inputs as TI                                    # noqa: E402
import verifiertraincommon as TC                                      # noqa: E402  (window / margin helpers of the tests)
import signature_verifier_train as R                                  # noqa: E402  (the reference)


class FixedMask(torch.nn.Module):
    """Stands where a Dropout stood: multiplies call k's input by the k-th multiplier."""

    def __init__(self):
        super().__init__()
        self.queue = []

    def forward(self, x):
        return x * self.queue.pop(0)


def run_case(n_pairs, e, steps, use_contrastive, dt, tag, out, prefix, record_decisions):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in VI.gen_state(e).items()}
    model = R.SiameseNetwork(embedding_dim=e)
    model.load_state_dict(sd, strict=True)
    model = model.to(dt).train()
    model.encoder.dropout = FixedMask()
    model.classifier[2] = FixedMask()
    opt = torch.optim.Adam(model.parameters(), lr=TI.LR)
    bce_fn, con_fn = torch.nn.BCELoss(), R.ContrastiveLoss(margin=2.0)
    taps = {}
    for i in (1, 2, 3):
        getattr(model.encoder, f"bn{i}").register_forward_hook((lambda k: lambda m, a, o: taps.setdefault(k, []).append(o.detach()))(f"route{i}"))
    model.encoder.fc1.register_forward_hook(lambda m, a, o: taps.setdefault("fc1_mask", []).append(o.detach()))
    model.classifier[0].register_forward_hook(lambda m, a, o: taps.setdefault("cls_mask", []).append(o.detach()))
    x1, x2 = torch.from_numpy(VI.gen_x1(n_pairs)).to(dt), torch.from_numpy(VI.gen_x2(n_pairs)).to(dt)
    y = torch.from_numpy(TI.labels(n_pairs)).to(dt)
    for step in range(steps):
        taps.clear()
        fk, ck = torch.from_numpy(TI.fc_keep(n_pairs, step)).to(dt), torch.from_numpy(TI.cls_keep(n_pairs, step)).to(dt)
        model.encoder.dropout.queue = [fk[:n_pairs] / (1.0 - TI.P_FC), fk[n_pairs:] / (1.0 - TI.P_FC)]
        model.classifier[2].queue = [ck / (1.0 - TI.P_CLS)]
        # the reference's train_epoch body (signature_verifier_train.py:413-438)
        opt.zero_grad()
        e1, e2, sim = model(x1, x2)
        bce = bce_fn(sim.squeeze(), y)
        if use_contrastive:
            con = con_fn(e1, e2, y)
            loss = bce + 0.5 * con
        else:
            con, loss = torch.zeros((), dtype=dt), bce
        loss.backward()
        opt.step()
        pred = (sim.squeeze() > 0.5).to(dt)
        k = f"{prefix}s{step}_"
        put = lambda name, t: out.__setitem__(f"{k}{name}_{tag}", np.array(t.detach().numpy()))
        put("loss", loss); put("bce", bce); put("contrastive", con); put("n_correct", (pred == y).sum().to(dt))
        put("e1", e1); put("e2", e2); put("similarity", sim.squeeze(1))
        put("distance", torch.nn.functional.pairwise_distance(e1, e2))
        for name, p in model.named_parameters():
            st = opt.state[p]
            out[f"{k}grad:{name}_{tag}"] = TI.pick(p.grad.numpy(), name)
            out[f"{k}param:{name}_{tag}"] = TI.pick(p.detach().numpy(), name)
            out[f"{k}exp_avg:{name}_{tag}"] = TI.pick(st["exp_avg"].numpy(), name)
            out[f"{k}exp_avg_sq:{name}_{tag}"] = TI.pick(st["exp_avg_sq"].numpy(), name)
        for name in TI.running_names():
            put(name, model.state_dict()[name])
        dec = {}
        for name in TI.DECISIONS if prefix == "" else ():        # the forward, and so every decision, is the same without the contrastive term
            z = torch.cat(taps[name], dim=0)
            dec[name] = (TC.route_of(z) if name.startswith("route") else (z > 0).to(torch.uint8)).numpy()
            if record_decisions:
                m = (TC.route_margin(z) if name.startswith("route") else TC.mask_margin(z)).reshape(-1).numpy()
                out[f"{k}{name}"] = dec[name]
                out[f"{k}tie:{name}"] = np.nonzero(m < TI.NEAR_TIE)[0].astype(np.int32)
            else:
                diff = int((dec[name] != out[f"{k}{name}"]).sum())
                print(f"  {k}{name}: fp32 decisions differ from fp64 in {diff} of {dec[name].size}; "
                      f"{out[f'{k}tie:{name}'].size} near ties listed")


def make_case(n_pairs, e, steps):
    out = {}
    variants = [("", True)] + ([("nc_", False)] if (n_pairs, e) == TI.NO_CONTRASTIVE else [])
    for prefix, use_c in variants:
        run_case(n_pairs, e, steps, use_c, torch.float64, "f64", out, prefix, True)
        run_case(n_pairs, e, steps, use_c, torch.float32, "f32", out, prefix, False)
    path = os.path.join(HERE, TI.case_name(n_pairs, e) + ".npz")
    np.savez_compressed(path, **out)
    keys = [k for k in out if k.endswith("_f64") and not ("conv" in k and ".bias" in k)]
    worst = max(float(np.abs(out[k[:-4] + "_f32"].astype(np.float64) - out[k]).max() / (np.abs(out[k]).max() + 1e-300)) for k in keys)
    print(f"case pairs={n_pairs} E={e}: {len(out)} arrays, {os.path.getsize(path)} bytes, worst fp32-vs-fp64 relative deviation "
          f"(conv biases aside) {worst:.2e}")


if __name__ == "__main__":
    torch.manual_seed(0)
    for n_pairs, e, steps, _ in TI.CASES:
        make_case(n_pairs, e, steps)
