"""Verifier train step, host side: the torch restatement (verifiertraincommon) against the reference's fixtures -- with the
fixture's decisions it reproduces the fp64 outputs, without forced decisions it takes them --, the pair dataset against the
reference's pair list, the checkpoint dictionary's keys and the new header's exports."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

import verifiertraincommon as TC
from verifiertraincommon import TI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
VARIANTS = [(n, e, steps, prefix, use_c) for n, e, steps, _ in TI.CASES
            for prefix, use_c in ([("", True)] + ([("nc_", False)] if (n, e) == TI.NO_CONTRASTIVE else []))]


def rel(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    scale = float(np.abs(want).max())
    return float(np.abs(got - want).max()) / scale if scale > 0 else float(np.abs(got).max())


def compare_step(f, k, out, P, m, v, R, P0, prev):
    """prev: the fixture key prefix of the step before (None at step 0).  The reference's conv biases walk by Adam-normalised
    rounding noise (about 1e-10 per step); the restatement's do not move.  That walk enters the reference's next running
    means directly -- the mean of conv + bias, weight 0.1 from x2 and 0.9 * 0.1 from x1 -- and is taken out of the
    expectation here, exactly, from the biases the fixture stores."""
    for name in ("loss", "bce", "contrastive", "n_correct", "e1", "e2", "similarity", "distance"):
        assert rel(out[name], f[f"{k}{name}_f64"]) <= TOL, name
    for name in P:
        if name in TC.CONV_BIAS:                          # mathematically zero: the reference's fp64 holds 1e-14 noise
            assert float(out["grads"][name].abs().max()) <= 1e-12
            continue
        assert rel(TI.pick(out["grads"][name].numpy(), name), f[f"{k}grad:{name}_f64"]) <= TOL, name
        assert rel(TI.pick(P[name].numpy(), name), f[f"{k}param:{name}_f64"]) <= TOL, name
        assert rel(TI.pick(m[name].numpy(), name), f[f"{k}exp_avg:{name}_f64"]) <= TOL, name
        assert rel(TI.pick(v[name].numpy(), name), f[f"{k}exp_avg_sq:{name}_f64"]) <= TOL, name
    for name in R:
        want = f[f"{k}{name}_f64"]
        if prev is not None and name.endswith("running_mean"):
            bias = name.replace("bn", "conv").replace("running_mean", "bias")
            want = want - 0.19 * (f[f"{prev}param:{bias}_f64"] - P0[bias].numpy())
        assert rel(R[name], want) <= TOL, name


@pytest.mark.parametrize("forced", [True, False])
@pytest.mark.parametrize("n_pairs,e,steps,prefix,use_c", VARIANTS)
def test_restatement_reproduces_the_fixture(n_pairs, e, steps, prefix, use_c, forced):
    f = TC.load_case(n_pairs, e)
    P, R = TC.state(e)
    P0 = {k: t.clone() for k, t in P.items()}
    m, v = TC.zero_moments(P)
    for step in range(steps):
        dec = TC.fixture_decisions(f, f"s{step}_")         # the forward is the same with and without the contrastive term
        out = TC.train_grads(P, R, TC.case_batch(n_pairs, step=step), use_c, decisions=dec if forced else None)
        if not forced:
            for name in TI.DECISIONS:
                assert torch.equal(out["decisions"][name], dec[name]), f"{name}: the restatement decides differently"
        with torch.no_grad():
            TC.adam_apply(P, out["grads"], m, v, step + 1)
        compare_step(f, f"{prefix}s{step}_", out, P, m, v, R, P0, f"{prefix}s{step - 1}_" if step else None)


def test_a_moved_route_moves_the_gradients():
    """The decisions are real inputs: one pool2 route moved by hand changes bn2's gradient by far more than the bound."""
    f = TC.load_case(2, 128)
    dec = TC.fixture_decisions(f, "s0_")
    P, R = TC.state(128)
    base = TC.train_grads(P, R, TC.case_batch(2), True, decisions=dec)
    r2 = dec["route2"].clone()
    flat = r2.view(-1)
    i = int(torch.nonzero(flat < 4)[0])
    flat[i] = (int(flat[i]) + 1) % 4
    P, R = TC.state(128)
    moved = TC.train_grads(P, R, TC.case_batch(2), True, decisions=dict(dec, route2=r2))
    assert rel(moved["grads"]["encoder.bn2.weight"], base["grads"]["encoder.bn2.weight"]) > 10 * TC.CAP


def test_fixture_sizes():
    biggest = max(os.path.getsize(os.path.join(TC.GOLDEN, n)) for n in os.listdir(TC.GOLDEN) if not n.startswith("golden_verifier_train"))
    for n_pairs, e, _, _ in TI.CASES:
        assert os.path.getsize(os.path.join(TC.GOLDEN, TI.case_name(n_pairs, e) + ".npz")) <= biggest


def test_library_exports_the_train_header():
    with open(os.path.join(ROOT, "include", "siggan_verifier_train.h")) as f:
        declared = set(re.findall(r"\b(?:int|int64_t)\s+(siggan_verifier_train\w+)\s*\(", f.read()))
    assert declared == {"siggan_verifier_trainer_create", "siggan_verifier_trainer_destroy", "siggan_verifier_trainer_param_count",
                        "siggan_verifier_trainer_param_span", "siggan_verifier_trainer_bind", "siggan_verifier_trainer_seed",
                        "siggan_verifier_train_grads", "siggan_verifier_train_apply", "siggan_verifier_train_step",
                        "siggan_verifier_train_debug"}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in siggan_verifier_train.h but not exported"
    assert declared == set(_lib.VERIFIER_TRAIN_EXPORTS)
    lib.siggan_abi_version.restype = C.c_int
    assert lib.siggan_abi_version() == 4                  # symbols only added


def write_users(root, users=3, sigs=3, seed=5):
    rng = np.random.default_rng(seed)
    for u in range(users):
        (root / f"user{u}").mkdir(parents=True)
        for k in range(sigs):
            a = np.where(rng.uniform(size=(48, 96)) < 0.1, rng.integers(0, 128, (48, 96)), 255).astype(np.uint8)
            Image.fromarray(a).save(str(root / f"user{u}" / f"sig{k}.png"))


def reference_pairs(user_signatures, pairs_per_user):
    """The pair list the reference's _generate_pairs draws (signature_verifier_train.py:318-346), as (i1, i2, label)
    names: random.sample / choice / shuffle in its order."""
    pairs = []
    ids = list(user_signatures)
    for u in ids:
        sigs = user_signatures[u]
        if u == "_synthetic_":
            continue
        for _ in range(pairs_per_user):
            if len(sigs) >= 2:
                a, b = random.sample(sigs, 2)
                pairs.append((a, b, 1))
        others = [o for o in ids if o != u]
        for _ in range(pairs_per_user):
            if others:
                o = random.choice(others)
                pairs.append((random.choice(sigs), random.choice(user_signatures[o]), 0))
    random.shuffle(pairs)
    return pairs


def test_pair_dataset_draws_the_reference_pairs(tmp_path, capsys):
    from signature_gan_amd import signature_verifier_train as ST
    data, syn = tmp_path / "real", tmp_path / "syn"
    write_users(data)
    syn.mkdir()
    Image.fromarray(np.full((64, 64), 200, np.uint8)).save(str(syn / "gen0.png"))
    random.seed(11)
    ds = ST.SignaturePairDataset(str(data), str(syn), pairs_per_user=4)
    text = capsys.readouterr().out
    assert "Loaded 4 users with signatures" in text and "  _synthetic_: 1 signatures" in text and "Generated 24 pairs" in text
    random.seed(11)
    want = reference_pairs(ds.user_signatures, 4)
    assert ds.pairs == want and len(ds) == 24
    assert sum(lab for _, _, lab in ds.pairs) == 12
    assert all("syn" not in str(a) for a, _, _ in ds.pairs)         # the synthetic user is only ever the second image
    x1, x2, y = ds[0]
    assert x1.shape == (1, 64, 64) and x1.dtype == torch.float32 and y.dtype == torch.float32
    # flat layout: the user is the file name's prefix
    flat = tmp_path / "flat"
    flat.mkdir()
    for u in ("a", "b"):
        for k in range(2):
            Image.fromarray(np.full((10, 10), 255, np.uint8)).save(str(flat / f"{u}_{k}.png"))
    assert set(ST.SignaturePairDataset(str(flat), pairs_per_user=1).user_signatures) == {"a", "b"}


def test_checkpoint_dictionary_and_module_surface():
    from signature_gan_amd import signature_verifier_train as ST
    model = ST.SiameseNetwork(embedding_dim=40)
    ck = ST.checkpoint_dict(model, 40, 0.75, 3, includes_synthetic=True)
    assert list(ck) == ["model_state_dict", "embedding_dim", "val_accuracy", "epoch", "includes_synthetic"]
    assert list(ST.checkpoint_dict(model, 40, 0.75, 3)) == ["model_state_dict", "embedding_dim", "val_accuracy", "epoch"]
    man = {k: tuple(s) for k, s, _ in TC.VC.load_manifest()["40"]}
    assert {k: tuple(v.shape) for k, v in ck["model_state_dict"].items()} == man
    assert [n for n, _ in model.named_parameters()] == TI.param_names(40)
    for name in ("CNNEncoder", "SiameseNetwork", "ContrastiveLoss", "SignaturePairDataset", "train_epoch", "evaluate", "train_model", "main"):
        assert hasattr(ST, name)
    e1, e2 = torch.tensor([[1.0, 0.0], [0.0, 1.0]]), torch.tensor([[1.0, 0.0], [1.0, 0.0]])
    d = torch.nn.functional.pairwise_distance(e1, e2)
    y = torch.tensor([1.0, 0.0])
    want = (y * d ** 2 + (1 - y) * torch.clamp(2.0 - d, min=0) ** 2).mean()
    assert float(ST.ContrastiveLoss(2.0)(e1, e2, y)) == float(want)
    with pytest.raises(RuntimeError):                     # no CPU path
        model.train().train_step(torch.zeros(1, 1, 64, 64), torch.zeros(1, 1, 64, 64), torch.ones(1), None)
    with pytest.raises(RuntimeError):
        ST.train_model("x", None, 1, "y", device="cpu")
