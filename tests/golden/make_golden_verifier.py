"""Fixtures of the Siamese signature verifier, made by running the REFERENCE's own SiameseNetwork
(signature_verifier_eval.py:39-179) on the CPU.  Run once where the reference is checked out; the outputs are committed:

    python tests/golden/make_golden_verifier.py

Nothing of the reference is copied: its module is imported at run time, fed the synthetic state and inputs of
verifier_inputs.py, and only its OUTPUTS are stored.

  golden_verifier_p<pairs>_e<E>.npz   per case: e1 / e2 / similarity of the reference in fp32 ("_f32") and of the same module
                                      in fp64 ("_f64"); at 64 fixed probe positions (inputs.probe_idx on the flattened
                                      (2 * pairs, ...) tensor, x1's images first) the three pooled activations and the
                                      fc1 output after ReLU, taken with forward hooks, in both precisions
  golden_verifier_metrics.npz         the reference's compute_verification_metrics / compute_eer_from_scores on
                                      verifier_inputs.gen_scores()
  verifier_manifest.json              the reference's state_dict keys / shapes / dtypes for E = 128 and 40
"""
import json
import os
import sys
import types

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/src")

import numpy as np                                                    # noqa: E402
import torch                                                          # noqa: E402
import torch.nn.functional as F                                       # noqa: E402

# the reference module imports torchvision at the top (only its dataset's default transform uses it); an empty stand-in
# is enough for the model classes and the metrics
if "torchvision" not in sys.modules:
    tv = types.ModuleType("torchvision")
    tv.transforms = types.ModuleType("torchvision.transforms")
    tv.transforms.Compose = object
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms

import inputs as I                                                    # noqa: E402
import verifier_inputs as VI                                          # noqa: E402
import signature_verifier_eval as R                                   # noqa: E402  (the reference)


def run(model, x1, x2):
    taps = {}
    hooks = []
    for name in ("pool1", "pool2", "pool3", "fc1"):
        taps[name] = []
        fn = (lambda n: lambda m, i, o: taps[n].append(F.relu(o.detach()) if n == "fc1" else o.detach()))(name)
        hooks.append(getattr(model.encoder, name).register_forward_hook(fn))
    with torch.no_grad():
        e1, e2, s = model(x1, x2)
    for h in hooks:
        h.remove()
    return e1, e2, s, {k: torch.cat(v, dim=0) for k, v in taps.items()}       # encoder ran on x1, then on x2


def make_case(n_pairs, e):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in VI.gen_state(e).items()}
    x1, x2 = torch.from_numpy(VI.gen_x1(n_pairs)), torch.from_numpy(VI.gen_x2(n_pairs))
    out = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        model = R.SiameseNetwork(embedding_dim=e)
        model.load_state_dict(sd, strict=True)
        model = model.to(dt).eval()
        e1, e2, s, taps = run(model, x1.to(dt), x2.to(dt))
        out[f"e1_{tag}"], out[f"e2_{tag}"], out[f"similarity_{tag}"] = e1.numpy(), e2.numpy(), s.numpy()
        for name, t in taps.items():
            a = t.reshape(-1).numpy()
            out[f"{name}_{tag}"] = a[I.probe_idx(a.size, "verifier:" + name)]
    np.savez_compressed(os.path.join(HERE, VI.case_name(n_pairs, e) + ".npz"), **out)
    d = lambda k: float(np.abs(out[k + "_f32"].astype(np.float64) - out[k + "_f64"]).max())
    print(f"case pairs={n_pairs} E={e}: fp32-vs-fp64 e1 {d('e1'):.2e} e2 {d('e2'):.2e} score {d('similarity'):.2e}; scores "
          f"{out['similarity_f64'].min():.3f}..{out['similarity_f64'].max():.3f}, max |e| {np.abs(out['e1_f64']).max():.3f}")


def make_metrics():
    y, s, thr = VI.gen_scores()
    pred = (s >= thr).astype(int)
    m = R.compute_verification_metrics(y, s, pred, thr)
    eer, eer_thr = R.compute_eer_from_scores(y, s)
    fpr, tpr, thrs = R.roc_curve(y, s)
    np.savez_compressed(os.path.join(HERE, "golden_verifier_metrics.npz"), metrics=json.dumps(m), eer=np.float64(eer),
                        eer_threshold=np.float64(eer_thr), fpr=fpr, tpr=tpr, thresholds=thrs)
    print(f"metrics: {len(fpr)} ROC points of {len(np.unique(s))} distinct scores; {m}")


def make_manifest():
    man = {}
    for e in (128, 40):
        sd = R.SiameseNetwork(embedding_dim=e).state_dict()
        man[str(e)] = [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
    with open(os.path.join(HERE, "verifier_manifest.json"), "w") as f:
        json.dump(man, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    torch.manual_seed(0)
    make_manifest()
    make_metrics()
    for n_pairs, e in VI.CASES:
        make_case(n_pairs, e)
