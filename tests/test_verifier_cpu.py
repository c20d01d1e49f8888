"""Signature verifier, host side: the C ABI's exports, the drop-in module's state_dict, its refusals, the numpy metrics
against the reference's (fixture), the test dataset, and the torch restatement (verifiercommon) against every fixture case."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_verifier_header():
    with open(os.path.join(ROOT, "include", "siggan_verifier.h")) as f:
        declared = set(re.findall(r"\bint\s+(siggan_verifier_\w+)\s*\(", f.read()))
    assert declared == {"siggan_verifier_create", "siggan_verifier_destroy", "siggan_verifier_bind", "siggan_verifier_embed",
                        "siggan_verifier_compare", "siggan_verifier_score", "siggan_verifier_debug_tensor"}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in siggan_verifier.h but not exported"
        assert name in _lib.VERIFIER_EXPORTS
    assert declared == set(_lib.VERIFIER_EXPORTS)
    lib.siggan_abi_version.restype = C.c_int
    assert lib.siggan_abi_version() == 4


@pytest.mark.parametrize("e", [128, 40])
def test_state_dict_matches_the_reference(e):
    want = VC.load_manifest()[str(e)]
    sd = SV.SiameseNetwork(e).state_dict()
    assert [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()] == want
    assert [k for k in VI.state_specs(e)] == [k for k, _, _ in want]
    # a reference checkpoint's state loads strictly
    SV.SiameseNetwork(e).load_state_dict(VC.torch_state(e), strict=True)


def test_forward_refuses_training_mode_and_cpu_tensors():
    m = SV.SiameseNetwork(128)
    x = torch.zeros(2, 1, 64, 64)
    with pytest.raises(RuntimeError, match="eval"):
        m(x, x)                                   # modules start in training mode
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_one(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.encoder(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SV.evaluate_signature_verifier("a.pth", None, ".", ".", device="cpu")


def test_cli_rejects_cpu(capsys):
    import sys
    argv = sys.argv
    sys.argv = ["signature_verifier_eval", "--baseline_model", "a.pth", "--test_dir", ".", "--device", "cpu"]
    try:
        with pytest.raises(SystemExit):
            SV.main()
    finally:
        sys.argv = argv
    assert "no CPU path" in capsys.readouterr().err


def _fixture_metrics():
    f = np.load(os.path.join(VC.GOLDEN, "golden_verifier_metrics.npz"))
    return f, json.loads(str(f["metrics"]))


def test_metrics_equal_the_reference():
    f, want = _fixture_metrics()
    y, s, thr = VI.gen_scores()
    fpr, tpr, thrs = SV.roc_curve(y, s)
    assert len(fpr) < len(np.unique(s)) + 1, "the score vector must exercise the dropping of collinear points"
    for got, name in ((fpr, "fpr"), (tpr, "tpr"), (thrs, "thresholds")):
        assert got.shape == f[name].shape and np.array_equal(got, f[name]), name
    got = SV.compute_verification_metrics(y, s, (s >= thr).astype(int), thr)
    assert list(got) == list(want)
    for k, v in want.items():
        if isinstance(v, int):
            assert isinstance(got[k], int) and got[k] == v, k
        else:
            assert isinstance(got[k], float) and abs(got[k] - v) <= 1e-12, (k, got[k], v)
    eer, eer_thr = SV.compute_eer_from_scores(y, s)
    assert abs(eer - float(f["eer"])) <= 1e-12 and abs(eer_thr - float(f["eer_threshold"])) <= 1e-12
    assert abs(eer - want["eer"]) <= 1e-12 and abs(eer_thr - want["eer_threshold"]) <= 1e-12


def test_metrics_edge_cases():
    """The reference's guards give 0.0 for a zero denominator.  With a class that has no samples at all the reference does
    not return: its ROC is all-NaN and np.nanargmin raises ValueError ("All-NaN slice encountered"; observed by running the
    reference on all-genuine and all-forgery labels) -- the same here.  The guards that can be reached are checked on
    predictions that leave a denominator empty."""
    s = np.array([0.1, 0.4, 0.6, 0.7, 0.2, 0.9])
    for y in (np.ones(6), np.zeros(6)):
        with pytest.raises(ValueError, match="All-NaN"):
            SV.compute_verification_metrics(y, s, (s >= 0.5).astype(int))
        with pytest.raises(ValueError, match="All-NaN"):
            SV.compute_eer_from_scores(y, s)
        fpr, tpr, _ = SV.roc_curve(y, s)
        assert np.isnan(fpr).all() if y[0] == 1 else np.isnan(tpr).all()
    y = np.array([1, 0, 1, 0, 1, 0.0])
    m = SV.compute_verification_metrics(y, s, np.zeros(6, int))          # nothing accepted: tp + fp = 0
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["f1_score"] == 0.0 and m["far"] == 0.0 and m["frr"] == 1.0
    m = SV.compute_verification_metrics(y, s, np.ones(6, int))
    assert m["specificity"] == 0.0 and m["far"] == 1.0 and m["frr"] == 0.0


def _write_users(root, layout):
    rng = np.random.default_rng(3)
    for u in range(3):
        for k in range(3):
            a = rng.integers(0, 256, (40 + 7 * u, 90 + 5 * k), dtype=np.uint8)
            if layout == "dirs":
                os.makedirs(os.path.join(root, f"user{u}"), exist_ok=True)
                p = os.path.join(root, f"user{u}", f"sig{k}.png")
            else:
                p = os.path.join(root, f"user{u}_{k}.png")
            Image.fromarray(a).save(p)


@pytest.mark.parametrize("layout", ["dirs", "flat"])
@pytest.mark.parametrize("ppu", [2, 5])
def test_dataset(tmp_path, layout, ppu):
    _write_users(str(tmp_path), layout)
    ds = SV.SignatureTestDataset(str(tmp_path), pairs_per_user=ppu)
    assert len(ds.user_signatures) == 3
    labels = [l for _, _, l in ds.pairs]
    assert set(labels) <= {0, 1}
    assert labels.count(1) == 3 * min(ppu, 3) and labels.count(0) == 3 * ppu       # n (n - 1) / 2 = 3 genuine at most
    # the same np.random calls in the same order: a second dataset draws the same pairs
    assert SV.SignatureTestDataset(str(tmp_path), pairs_per_user=ppu).pairs == ds.pairs
    a, b, l = ds[0]
    assert a.shape == (1, 64, 64) and a.dtype == torch.float32 and l.dtype == torch.float32
    p1, p2, _ = ds.pairs[0]
    for got, path in ((a, p1), (b, p2)):
        u8 = np.asarray(Image.open(path).convert("L").resize((64, 64), Image.BILINEAR), dtype=np.uint8)
        want = (u8.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
        assert np.array_equal(got.numpy()[0], want)
    ua, ub, ul = ds.get_uint8(0)
    assert ua.dtype == torch.uint8 and ua.shape == (64, 64) and float(ul) == float(l)
    assert np.array_equal(SV.normalize_uint8(ua.numpy()), a.numpy()[0]) and np.array_equal(SV.normalize_uint8(ub.numpy()), b.numpy()[0])
    du = SV.SignatureTestDataset(str(tmp_path), pairs_per_user=ppu, uint8=True)
    assert du.pairs == ds.pairs and torch.equal(du[0][0], ua)


@pytest.mark.parametrize("n_pairs,e", VI.CASES)
def test_restatement_reproduces_the_fixture(n_pairs, e):
    f = VC.load_case(n_pairs, e)
    x1, x2, b2 = VC.case_inputs(n_pairs)
    assert np.array_equal(VI.normalize_bytes(b2.numpy())[:, None], x2.numpy())
    taps = {}
    e1, e2, s = VC.forward(VC.torch_state(e), x1, x2, taps)
    what = f"restatement pairs={n_pairs} E={e}"
    VC.check(e1.numpy(), f, "e1", what)
    VC.check(e2.numpy(), f, "e2", what)
    VC.check(s.numpy(), f, "similarity", what)
    for name, shape in VI.STAGES:
        assert tuple(taps[name].shape) == (2 * n_pairs,) + shape
        VC.check(VC.probe(taps[name], name), f, name, what)
