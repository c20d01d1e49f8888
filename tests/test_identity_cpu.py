"""Host side of identity-guided projection (no GPU): the fp64 restatement of the verifier's eval-mode input gradient equals
torch.autograd on verifiercommon.encode / head when it takes its own decisions, its synthetic inputs are not vacuous, the
host-side refusals raise before anything is allocated, a projection with both identity weights 0 never touches the verifier,
and the new entry points are declared, listed and exported."""
import os
import re

import numpy as np
import pytest
import torch

from common import ROOT

import identitycommon as IC
import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.generate_signatures import parse_args
from signature_gan_amd.generator_vanilla_gan import Generator
from signature_gan_amd.signature_verifier_eval import SiameseNetwork
from signature_gan_amd.utils import inference


@pytest.fixture(scope="module")
def runs():
    """(E) -> (sd, x, r): N = 3 images and the fp64 embeddings of three targets."""
    out = {}
    for e in (128, 40):
        sd = IC.identity_state(e)
        x, t = IC.images(3)
        with torch.no_grad():
            r = IC.VC.encode(sd, t.double())
        out[e] = (sd, x, r)
    return out


@pytest.mark.parametrize("w", IC.WEIGHTS, ids=lambda w: f"we{w[0]}_ws{w[1]}")
@pytest.mark.parametrize("e", [128, 40])
def test_restatement_with_its_own_decisions_is_autograd(runs, e, w):
    sd, x, r = runs[e]
    assert float(sd["encoder.bn2.weight"][IC.GAMMA_NEG]) < 0 and float(sd["encoder.bn2.weight"][IC.GAMMA_ZERO]) == 0
    out = IC.input_grad_ref(sd, x, r, *w)
    dx, obj = IC.autograd_ref(sd, x, r, *w)
    scale = float(dx.abs().max())
    assert scale > 0
    d = float((out["dx"] - dx).abs().max()) / scale
    print(f"E {e} weights {w}: |dx - autograd| / max|dx| = {d:.3e}, max|dx| = {scale:.3e}")
    assert d <= 1e-12
    assert float((out["objective"] - obj).abs().max()) <= 1e-12 * float(obj.abs().max())
    want = w[0] * out["terms"][0] + w[1] * out["terms"][1]
    assert torch.allclose(out["objective"], want, rtol=1e-14, atol=0)
    for k, wk in enumerate(w):                                           # a term whose weight is 0 is reported as 0
        assert (float(out["terms"][k].abs().max()) == 0) == (wk == 0)
    # given back its own decisions it reproduces itself
    again = IC.input_grad_ref(sd, x, r, *w, decisions=out["decisions"])
    assert torch.equal(again["dx"], out["dx"])


@pytest.mark.parametrize("e", [128, 40])
def test_synthetic_inputs_are_not_vacuous(e):
    """What the GPU test asserts of the device's run holds for the fp64 run of the same inputs at every N it uses."""
    sd = IC.identity_state(e)
    x, t = IC.images(65)
    with torch.no_grad():
        r = IC.VC.encode(sd, t.double())
    out = IC.input_grad_ref(sd, x, r, 0.5, 2.0)
    dead = IC.dead_fraction(out["decisions"])
    print(f"E {e}: dead {dead}, max|logit| {float(out['logit'].abs().max()):.3f}, max|dx| {float(out['dx'].abs().max()):.3e}")
    assert float(out["dx"].abs().max()) > 0
    assert float(out["logit"].abs().max()) < 6
    assert all(v < 0.9 for v in dead.values())
    g = out["dx"].reshape(65, -1).abs().amax(dim=1)
    assert float(g.min()) > 0                                            # every image has a gradient


def test_input_grad_refusals_raise_before_any_allocation():
    model = SiameseNetwork(embedding_dim=40, max_images=4).eval()        # on the CPU: reaching the device path raises RuntimeError
    x, r = torch.zeros(2, 1, 64, 64), torch.zeros(2, 40)
    for bad in (dict(embed_weight=-1.0), dict(embed_weight=float("nan")), dict(embed_weight=0.0, score_weight=0.0),
                dict(score_weight=float("inf"))):
        with pytest.raises(ValueError):
            model.input_grad(x, r, **bad)
    with pytest.raises(ValueError):
        model.input_grad(torch.zeros(2, 1, 32, 32), r)
    with pytest.raises(ValueError):
        model.input_grad(x, torch.zeros(2, 41))
    with pytest.raises(ValueError):
        model.input_grad(x.double(), r)
    with pytest.raises(ValueError):
        model.input_grad(torch.zeros(5, 1, 64, 64), torch.zeros(5, 40))  # more than max_images
    with pytest.raises(ValueError):
        model.input_grad(x, r, dx_out=torch.zeros(3))
    assert model._ctx is None                                            # nothing was created
    with pytest.raises(RuntimeError):                                    # valid arguments: there is no CPU path
        model.input_grad(x, r)


class _Poison:
    """A verifier nobody may look at."""

    def __getattr__(self, name):
        raise AssertionError(f"the verifier was touched: .{name}")


def test_projection_refusals_raise_before_any_allocation():
    g64, g128 = Generator(100, 64).eval(), Generator(100, 128).eval()
    verifier = SiameseNetwork(embedding_dim=40).eval()
    t = np.zeros((1, 64, 64), dtype=np.uint8)
    with pytest.raises(ValueError, match="need the verifier"):
        inference.project_signatures(g64, t, steps=1, identity_weight=1.0)
    with pytest.raises(ValueError, match="64x64"):
        inference.project_signatures(g128, np.zeros((1, 128, 128), dtype=np.uint8), steps=1, verifier=verifier, identity_weight=1.0)
    for bad in (dict(identity_weight=-1.0), dict(identity_score_weight=-0.5), dict(identity_weight=float("nan"))):
        with pytest.raises(ValueError, match="identity weights"):
            inference.project_signatures(g64, t, steps=1, verifier=verifier, **bad)
    with pytest.raises(ValueError, match="eval"):
        inference.project_signatures(g64, t, steps=1, verifier=SiameseNetwork(embedding_dim=40), identity_score_weight=1.0)
    meta = SiameseNetwork(embedding_dim=40).eval().to("meta")            # a verifier on another device
    with pytest.raises(ValueError, match="one device"):
        inference.project_signatures(g64, t, steps=1, verifier=meta, identity_weight=1.0)
    assert g64._engine is None and verifier._ctx is None


class _FakeEngine:
    """The Engine calls a pixel-only projection makes, on the CPU: the objective is sum z^2, nothing else."""
    device, latent_dim, image_size, max_batch = torch.device("cpu"), 100, 64, 8

    def __init__(self):
        self.calls = []

    def g_latent_objective_grad(self, z, target, wr, wd, wp, dz_out=None, objective_out=None, **kw):
        self.calls.append(sorted(kw))
        dz_out.copy_(2 * z)
        if objective_out is not None:
            objective_out.copy_((z * z).sum(dim=1))

    def op_adam(self, z, dz, m, v, t, lr, beta1, beta2):
        z -= lr * dz


def test_zero_identity_weights_never_touch_the_verifier(monkeypatch):
    g = Generator(100, 64).eval()
    eng = _FakeEngine()
    monkeypatch.setattr(g, "_require_engine", lambda: eng)
    monkeypatch.setattr(inference, "generate_uint8", lambda gen, z: np.zeros((z.shape[0], 64, 64), dtype=np.uint8))
    t = np.zeros((2, 64, 64), dtype=np.uint8)
    want = inference.project_signatures(g, t, steps=3, seed=1)
    got = inference.project_signatures(g, t, steps=3, seed=1, verifier=_Poison(), identity_weight=0.0, identity_score_weight=0.0)
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert all("image_grad" not in c for c in eng.calls)                 # the unseeded call, with the arguments it always had


def test_cli_takes_the_identity_flags_and_keeps_the_namespace():
    a = vars(parse_args(["--checkpoint", "g.pt", "--project", "dir"]))
    assert not any(k in a for k in ("verifier_checkpoint", "project_identity_weight", "project_identity_score_weight"))
    a = parse_args(["--checkpoint", "g.pt", "--project", "dir", "--verifier_checkpoint", "v.pth", "--project_identity_weight", "0.5",
                    "--project_identity_score_weight", "2"])
    assert (a.verifier_checkpoint, a.project_identity_weight, a.project_identity_score_weight) == ("v.pth", 0.5, 2.0)
    assert parse_args(["--checkpoint", "g.pt", "--project", "dir", "--verifier_checkpoint", "v.pth"]).verifier_checkpoint == "v.pth"
    for bad in (["--verifier_checkpoint", "v.pth"],                                            # needs --project
                ["--project", "dir", "--project_identity_weight", "1"],                        # needs the verifier
                ["--project", "dir", "--verifier_checkpoint", "v.pth", "--project_identity_weight", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(["--checkpoint", "g.pt"] + bad)


def test_entry_points_are_declared_listed_and_exported():
    vh = open(os.path.join(ROOT, "include", "siggan_verifier_grad.h")).read()
    gh = open(os.path.join(ROOT, "include", "siggan.h")).read()
    assert re.search(r"int siggan_verifier_input_grad_enable\(siggan_verifier \*v\)", vh)
    decl = re.search(r"int siggan_verifier_input_grad\(([^;]*)\);", vh)
    assert decl and len(re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")) == 11
    decl = re.search(r"int siggan_g_latent_objective_grad_seeded\(([^;]*)\);", gh)
    assert decl and len(decl.group(1).split(",")) == 13
    assert "#define SIGGAN_ABI_VERSION 4" in gh                              # new symbols only
    lib = _lib.load()
    for name in ("siggan_verifier_input_grad_enable", "siggan_verifier_input_grad", "siggan_verifier_input_grad_debug"):
        assert name in _lib.VERIFIER_GRAD_EXPORTS and hasattr(lib, name)
    assert set(re.findall(r"\bint\s+(siggan_verifier_\w+)\s*\(", vh)) == set(_lib.VERIFIER_GRAD_EXPORTS)
    assert "siggan_g_latent_objective_grad_seeded" in _lib.EXPORTS
    assert len(lib.siggan_g_latent_objective_grad_seeded.argtypes) == 13
    assert lib.siggan_verifier_input_grad_enable(None) == _lib.E_ARG        # a null context: refused
    assert lib.siggan_verifier_input_grad(None, None, None, 1, None, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.siggan_g_latent_objective_grad_seeded(None, None, 1, None, None, None, None, None, None, None, None, None, None) == -1
