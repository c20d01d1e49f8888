"""Signature verifier on the MI355X: the C ABI (siggan_verifier.h) and the drop-in module against the reference's fixtures
(tests/golden/golden_verifier_*.npz) and the torch restatement (verifiercommon), plus the bitwise properties of the path.
The bound is verifiercommon's: 32 x the reference's own fp32-vs-fp64 deviation, never looser than 1e-4."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cuda(t):
    return t.to(DEV)


def weights_of(sd):
    """The 26 tensors of _lib.VERIFIER_WEIGHT_FIELDS from a reference state dict, on the device."""
    out = []
    for i in (1, 2, 3):
        out += [sd[f"encoder.conv{i}.weight"], sd[f"encoder.conv{i}.bias"], sd[f"encoder.bn{i}.weight"], sd[f"encoder.bn{i}.bias"],
                sd[f"encoder.bn{i}.running_mean"], sd[f"encoder.bn{i}.running_var"]]
    out += [sd[k] for k in ("encoder.fc1.weight", "encoder.fc1.bias", "encoder.fc2.weight", "encoder.fc2.bias",
                            "classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias")]
    return [cuda(t) for t in out]


def make_ctx(e, max_images, seed=VI.SEED["state"]):
    ctx = SV._Context(DEV, e, max_images)
    ctx.bind(weights_of(VC.torch_state(e, seed)), VC.BN_EPS)
    return ctx


@functools.lru_cache(maxsize=None)
def shared_ctx(e):
    return make_ctx(e, 66)


def make_model(e, seed=VI.SEED["state"], max_images=SV.DEFAULT_MAX_IMAGES):
    m = SV.SiameseNetwork(e, max_images=max_images)
    m.load_state_dict(VC.torch_state(e, seed), strict=True)
    return m.to(DEV).eval()


def bound_vs(ref32, ref64):
    """verifiercommon's bound for a tensor without a fixture: the restatement's own fp32-vs-fp64 deviation takes the
    fixture's place (absolute: embeddings and scores)."""
    return min(VC.MARGIN * float((ref32.double() - ref64).abs().max()), VC.CAP)


@pytest.mark.parametrize("n_pairs,e", VI.CASES)
def test_fixture_case(n_pairs, e):
    f = VC.load_case(n_pairs, e)
    x1, x2, _ = VC.case_inputs(n_pairs)
    ctx = shared_ctx(e)
    e1, e2, s = ctx.score(cuda(x1), cuda(x2))
    what = f"hip pairs={n_pairs} E={e}"
    stages = {name: ctx.debug_tensor(name, (2 * n_pairs,) + shape).cpu() for name, shape in VI.STAGES}
    for name, _ in VI.STAGES:                             # in network order: the first failure names the layer
        VC.check(VC.probe(stages[name], name), f, name, what)
    VC.check(e1.cpu().numpy(), f, "e1", what)
    VC.check(e2.cpu().numpy(), f, "e2", what)
    VC.check(s.cpu().numpy(), f, "similarity", what)
    assert s.shape == (n_pairs, 1)
    nrm = torch.cat([e1, e2]).double().norm(dim=1).cpu()
    assert float((nrm - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("n_pairs,e", [(3, 128), (33, 128), (3, 40)])
def test_embed_then_compare_equals_score_bitwise(n_pairs, e):
    x1, x2, _ = VC.case_inputs(n_pairs)
    ctx = shared_ctx(e)
    e1, e2, s = ctx.score(cuda(x1), cuda(x2))
    g1, g2 = ctx.embed(cuda(x1)), ctx.embed(cuda(x2))
    assert torch.equal(g1, e1) and torch.equal(g2, e2)
    assert torch.equal(ctx.compare(g1, g2), s)
    # embeddings not asked for: the same scores
    s2 = torch.empty(n_pairs, dtype=torch.float32, device=DEV)
    a, b = cuda(x1).contiguous(), cuda(x2).contiguous()
    _lib.check(ctx.lib.siggan_verifier_score(ctx._h, SV._ptr(a), SV._ptr(b), _lib.VFMT_F32, n_pairs, None, None, SV._ptr(s2),
                                             ctx._stream()))
    assert torch.equal(s2, s[:, 0])


def test_byte_route_equals_fp32_route_bitwise():
    _, x2, b2 = VC.case_inputs(33)
    ctx = shared_ctx(128)
    assert torch.equal(ctx.embed(cuda(b2)), ctx.embed(cuda(x2)))
    p1 = ctx.debug_tensor("pool1", (33, 32, 32, 32)).clone()
    ctx.embed(cuda(b2))
    assert torch.equal(ctx.debug_tensor("pool1", (33, 32, 32, 32)), p1)
    a, b, s = ctx.score(cuda(b2[:16]), cuda(b2[16:32]))
    a2, b2f, s2 = ctx.score(cuda(x2[:16]), cuda(x2[16:32]))
    assert torch.equal(a, a2) and torch.equal(b, b2f) and torch.equal(s, s2)


def test_position_independence():
    x1, x2, _ = VC.case_inputs(3)
    ctx = shared_ctx(128)
    imgs = torch.cat([x1, x2])                            # 6 images
    imgs[3] = imgs[0]
    imgs[5] = imgs[0]
    e = ctx.embed(cuda(imgs))
    assert torch.equal(e[0], e[3]) and torch.equal(e[0], e[5])
    assert not torch.equal(e[0], e[1])
    # the same picture alone in a batch, and in a batch that fills more than one fc1 row tile
    assert torch.equal(ctx.embed(cuda(imgs[:1]))[0], e[0])
    big = torch.cat([VC.case_inputs(33)[0], imgs[:1].expand(33, -1, -1, -1)])
    assert torch.equal(ctx.embed(cuda(big))[65], e[0])
    # (x, x) scores sigmoid(head(0)) in every row
    _, _, s = ctx.score(cuda(imgs[:3]), cuda(imgs[:3]))
    z = torch.zeros(1, 128, device=DEV)
    s0 = ctx.compare(z, z)
    assert all(torch.equal(s[i], s0[0]) for i in range(3))
    sd = VC.torch_state(128, dtype=torch.float64)
    want = VC.head(sd, torch.zeros(1, 128, dtype=torch.float64), torch.zeros(1, 128, dtype=torch.float64))
    assert abs(float(s0) - float(want)) <= 1e-6


def test_chunked_call_through_the_module():
    f = VC.load_case(33, 128)
    x1, x2, _ = VC.case_inputs(33)
    m = make_model(128, max_images=8)                     # 4 pairs per call: 9 calls, the last of one pair
    e1, e2, s = m(cuda(x1), cuda(x2))
    what = "chunked pairs=33 E=128"
    VC.check(e1.cpu().numpy(), f, "e1", what)
    VC.check(e2.cpu().numpy(), f, "e2", what)
    VC.check(s.cpu().numpy(), f, "similarity", what)
    # chunking changes no bit: the sum order of a row depends neither on its position nor on the batch
    r1, r2, rs = shared_ctx(128).score(cuda(x1), cuda(x2))
    assert torch.equal(e1, r1) and torch.equal(e2, r2) and torch.equal(s, rs)
    assert torch.equal(m.forward_one(cuda(x1)), r1)


@pytest.mark.parametrize("e", [128, 40])
def test_dropin_checkpoint(tmp_path, e):
    path = str(tmp_path / "verifier.pth")
    torch.save({"model_state_dict": VC.torch_state(e), "embedding_dim": e, "val_accuracy": 0.9125, "epoch": 17,
                "includes_synthetic": True}, path)
    model, meta = SV.load_model(path, torch.device(DEV))
    assert meta == {"embedding_dim": e, "val_accuracy": 0.9125, "epoch": 17, "includes_synthetic": True, "checkpoint_path": path}
    assert not model.training and next(model.parameters()).device.type == "cuda"
    x1, x2, _ = VC.case_inputs(3)
    e1, e2, s = model(cuda(x1), cuda(x2))
    r1, r2, rs = shared_ctx(e).score(cuda(x1), cuda(x2))
    assert torch.equal(e1, r1) and torch.equal(e2, r2) and torch.equal(s, rs)
    assert torch.equal(model.encoder(cuda(x1)), r1)        # the bare encoder module
    with pytest.raises(RuntimeError, match="eval"):
        model.train()(cuda(x1), cuda(x2))


def test_packs_follow_load_state_dict():
    x1, x2, _ = VC.case_inputs(3)
    m = make_model(128)
    before = [t.clone() for t in m(cuda(x1), cuda(x2))]
    m.load_state_dict(VC.torch_state(128, VI.SEED["state2"]), strict=True)
    got = m(cuda(x1), cuda(x2))
    ref32 = VC.forward(VC.torch_state(128, VI.SEED["state2"]), x1, x2)
    ref64 = VC.forward(VC.torch_state(128, VI.SEED["state2"], torch.float64), x1.double(), x2.double())
    for name, g, r32, r64, old in zip(("e1", "e2", "similarity"), got, ref32, ref64, before):
        d, b = float((g.cpu().double() - r64).abs().max()), bound_vs(r32, r64)
        print(f"second state {name}: deviation {d:.3e} bound {b:.3e}")
        assert d <= b, f"{name}: deviation {d:.3e} exceeds bound {b:.3e} (stale packs?)"
        assert float((g - old).abs().max()) > 1e-3
    # in-place writes are picked up after params_changed()
    with torch.no_grad():
        m.classifier[3].bias.add_(1.0)
    assert torch.equal(m(cuda(x1), cuda(x2))[2], got[2])
    m.params_changed()
    assert float((m(cuda(x1), cuda(x2))[2] - got[2]).abs().min()) > 1e-2


def test_generated_bytes_score_end_to_end():
    from common import I, SEED
    from hipcommon import make_engine
    eng = make_engine(64, 100, 4)
    fake = eng.g_generate_u8(cuda(torch.from_numpy(I.gen_z(4, 100, SEED["z"]))))
    real = cuda(torch.from_numpy(VI.gen_x2_bytes(4, seed=77)))
    assert fake.dtype == torch.uint8 and fake.shape == (4, 64, 64)
    m = make_model(128)
    got = m.score_u8(fake, real)
    xf = torch.from_numpy(VI.normalize_bytes(fake.cpu().numpy()))[:, None]
    xr = torch.from_numpy(VI.normalize_bytes(real.cpu().numpy()))[:, None]
    ref32 = VC.forward(VC.torch_state(128), xf, xr)
    ref64 = VC.forward(VC.torch_state(128, dtype=torch.float64), xf.double(), xr.double())
    for name, g, r32, r64 in zip(("e1", "e2", "similarity"), got, ref32, ref64):
        d, b = float((g.cpu().double() - r64).abs().max()), bound_vs(r32, r64)
        print(f"generated bytes {name}: deviation {d:.3e} bound {b:.3e}")
        assert d <= b, f"{name}: deviation {d:.3e} exceeds bound {b:.3e}"
    assert torch.equal(m.embed_u8(fake), got[0]) and torch.equal(m.compare(got[0], got[1]), got[2])
    eng.close()


def test_evaluate_signature_verifier(tmp_path, capsys):
    rng = np.random.default_rng(5)
    data = tmp_path / "test"
    for u in range(3):
        (data / f"user{u}").mkdir(parents=True)
        for k in range(3):
            a = np.where(rng.uniform(size=(48, 96)) < 0.1, rng.integers(0, 128, (48, 96)), 255).astype(np.uint8)
            Image.fromarray(a).save(str(data / f"user{u}" / f"sig{k}.png"))
    path = str(tmp_path / "augmented.pth")
    torch.save({"model_state_dict": VC.torch_state(128), "embedding_dim": 128, "val_accuracy": 0.875, "epoch": 3,
                "includes_synthetic": True}, path)
    out = tmp_path / "out"
    report = SV.evaluate_signature_verifier(None, path, str(data), str(out), batch_size=4, pairs_per_user=3, device="cuda")
    with open(out / "evaluation_report.json") as f:
        on_disk = json.load(f)
    assert set(on_disk) == {"evaluation_timestamp", "num_models_evaluated", "models"} and list(on_disk["models"]) == ["Augmented"]
    rep = on_disk["models"]["Augmented"]
    assert set(rep) == {"model_metadata", "metrics", "num_test_samples", "genuine_samples", "forgery_samples"}
    assert rep["num_test_samples"] == 18 and rep["genuine_samples"] == 9 and rep["forgery_samples"] == 9
    assert rep["model_metadata"]["includes_synthetic"] is True and rep["metrics"] == report["models"]["Augmented"]["metrics"]
    text = capsys.readouterr().out
    assert "SIGNATURE VERIFICATION EVALUATION SUMMARY" in text and "[Report] Evaluation report saved to:" in text
    assert ("[Plot] ROC curve saved to:" in text) != ("[Plot] skipped (matplotlib not available)" in text)
    # the per-pair scores are those of a direct model() call on the same pairs, in the fp32 and in the byte route
    ds = SV.SignatureTestDataset(str(data), pairs_per_user=3)
    model = make_model(128)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)
    metrics, y_true, y_scores, y_pred = SV.evaluate_model(model, loader, torch.device(DEV))
    x1 = torch.stack([ds[i][0] for i in range(len(ds))])
    x2 = torch.stack([ds[i][1] for i in range(len(ds))])
    direct = model(cuda(x1), cuda(x2))[2][:, 0].cpu().numpy()
    assert np.array_equal(y_scores, direct.astype(np.float64))
    assert np.array_equal(y_true, np.array([ds[i][2].item() for i in range(len(ds))]))
    assert metrics == rep["metrics"]
    du = SV.SignatureTestDataset(str(data), pairs_per_user=3, uint8=True)
    _, _, u_scores, _ = SV.evaluate_model(model, torch.utils.data.DataLoader(du, batch_size=4), torch.device(DEV))
    assert np.array_equal(u_scores, y_scores)


def test_argument_errors_enqueue_nothing():
    lib = _lib.load()
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    x = torch.zeros(4, 1, 64, 64, device=DEV)
    emb = torch.full((4, 128), 7.0, device=DEV)
    sc = torch.full((4,), 7.0, device=DEV)
    p = SV._ptr

    def refused(rc, text):
        assert rc == _lib.E_ARG
        assert text in lib.siggan_last_error().decode()
        torch.cuda.synchronize()
        assert bool((emb == 7.0).all()) and bool((sc == 7.0).all())

    h = C.c_void_p()
    assert lib.siggan_verifier_create(0, 0, 4, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.siggan_verifier_create(0, 128, 0, C.byref(h)) == _lib.E_ARG and not h.value
    ctx = SV._Context(DEV, 128, 4)
    # before bind
    refused(lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 2, p(emb), st), "bind")
    refused(lib.siggan_verifier_score(ctx._h, p(x), p(x), _lib.VFMT_F32, 2, p(emb), p(emb), p(sc), st), "bind")
    refused(lib.siggan_verifier_compare(ctx._h, p(emb), p(emb), 2, p(sc), st), "bind")
    refused(lib.siggan_verifier_debug_tensor(ctx._h, b"fc1", p(emb), 512, st), "bind")
    ctx.bind(weights_of(VC.torch_state(128)), VC.BN_EPS)
    refused(lib.siggan_verifier_debug_tensor(ctx._h, b"fc1", p(emb), 512, st), "no embed")
    refused(lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 0, p(emb), st), "n_images")
    refused(lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 5, p(emb), st), "n_images")
    refused(lib.siggan_verifier_embed(ctx._h, p(x), 2, 2, p(emb), st), "fmt")
    refused(lib.siggan_verifier_embed(ctx._h, None, _lib.VFMT_F32, 2, p(emb), st), "null")
    refused(lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 2, None, st), "null")
    refused(lib.siggan_verifier_score(ctx._h, p(x), p(x), _lib.VFMT_F32, 3, p(emb), p(emb), p(sc), st), "n_pairs")
    refused(lib.siggan_verifier_score(ctx._h, p(x), p(x), _lib.VFMT_F32, 0, p(emb), p(emb), p(sc), st), "n_pairs")
    refused(lib.siggan_verifier_score(ctx._h, p(x), p(x), 7, 2, p(emb), p(emb), p(sc), st), "fmt")
    refused(lib.siggan_verifier_score(ctx._h, p(x), None, _lib.VFMT_F32, 2, p(emb), p(emb), p(sc), st), "null")
    refused(lib.siggan_verifier_compare(ctx._h, p(emb), None, 2, p(sc), st), "null")
    refused(lib.siggan_verifier_compare(ctx._h, p(emb), p(emb), 0, p(sc), st), "n_pairs")
    assert lib.siggan_verifier_bind(ctx._h, None, st) == _lib.E_ARG
    # the Python shim maps the code to ValueError
    with pytest.raises(ValueError):
        _lib.check(lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 9, p(emb), st))
    # and a good call still works afterwards
    assert lib.siggan_verifier_embed(ctx._h, p(x), _lib.VFMT_F32, 4, p(emb), st) == 0
    torch.cuda.synchronize()
    assert float((emb.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    refused_n = lib.siggan_verifier_debug_tensor(ctx._h, b"pool9", p(sc), 4, st)
    assert refused_n == _lib.E_ARG
    assert lib.siggan_verifier_debug_tensor(ctx._h, b"fc1", p(sc), 4, st) == _lib.E_ARG      # wrong element count
    ctx.close()
