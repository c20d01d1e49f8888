"""Hard-pair mining, host side: the selection on hand-made index arrays, the signature table, the trainer's flags and its
host-pipeline refusal, the host refusals of pair_topk, and the new header's exports."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import verifierdatacommon as DC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV
from signature_gan_amd import signature_verifier_train as ST
from signature_gan_amd import verifier_mining as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hard_pairs_from_topk():
    #            anchor: 0        1        2         3 (skipped)  4
    imp = np.array([[3, 4], [0, -1], [1, 0], [0, 1], [0, 2]], np.int32)
    gen = np.array([[1], [0], [-1], [4], [3]], np.int32)
    ok = np.array([True, True, True, False, True])
    got = VM.hard_pairs_from_topk(imp, gen, ok)
    # anchor 0: both impostors, its genuine partner; anchor 1: (1, 0) twice, both seen as (0, 1); the -1 is padding;
    # anchor 2: two new impostors, no genuine partner; anchor 3 is no anchor; anchor 4: (4, 0) is (0, 4), then new ones
    want = [(0, 3, 0), (0, 4, 0), (0, 1, 1), (2, 1, 0), (2, 0, 0), (4, 2, 0), (4, 3, 1)]
    assert got.dtype == np.int64 and got.shape == (7, 3) and got.tolist() == [list(w) for w in want]
    # exclusion is unordered and takes (i, j) or (i, j, label) rows
    got = VM.hard_pairs_from_topk(imp, gen, ok, exclude=[(3, 0), (1, 2, 0), (3, 4)])
    assert got.tolist() == [[0, 4, 0], [0, 1, 1], [2, 0, 0], [4, 2, 0]]
    # nothing to mine; k = 0 for a class
    none = VM.hard_pairs_from_topk(np.full((3, 2), -1), np.zeros((3, 0), np.int32), [True, False, True])
    assert none.shape == (0, 3) and none.dtype == np.int64
    assert VM.hard_pairs_from_topk(imp, gen, np.zeros(5, bool)).shape == (0, 3)
    with pytest.raises(ValueError):
        VM.hard_pairs_from_topk(imp[:4], gen, ok)


def test_signature_table(tmp_path, capsys):
    DC.write_users(tmp_path / "real")
    (tmp_path / "syn").mkdir()
    for k in range(4):
        DC.Image.fromarray(np.full((8, 8), 50 * k, np.uint8)).save(str(tmp_path / "syn" / f"g{k}.png"))
    random.seed(1)
    ds = ST.SignaturePairDataset(str(tmp_path / "real"), str(tmp_path / "syn"), pairs_per_user=2)
    capsys.readouterr()
    files, ids, synthetic = VM.signature_table(ds)
    users = list(ds.user_signatures)
    assert users[-1] == "_synthetic_" and len(files) == 13
    assert files == [p for u in users for p in ds.user_signatures[u]]
    assert ids.dtype == np.int32 and ids.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 4
    assert synthetic.dtype == bool and synthetic.tolist() == [False] * 9 + [True] * 4
    sub = torch.utils.data.Subset(torch.utils.data.Subset(ds, [5, 1, 2]), [2, 0])
    f2, i2, s2 = VM.signature_table(sub)                              # the table is the base dataset's, whatever the split
    assert f2 == files and np.array_equal(i2, ids) and np.array_equal(s2, synthetic)
    random.seed(1)
    plain = ST.SignaturePairDataset(str(tmp_path / "real"), None, pairs_per_user=2)
    capsys.readouterr()
    assert not VM.signature_table(plain)[2].any() and len(VM.signature_table(plain)[0]) == 9


def parse(monkeypatch, argv):
    seen = {}
    monkeypatch.setattr(ST, "train_model", lambda **kw: seen.update(kw) or {})
    ST.main(["--data_dir", "d"] + argv)
    return seen


def test_flags_only_when_given(monkeypatch, capsys):
    base = {"data_dir", "synthetic_dir", "epochs", "model_output", "batch_size", "learning_rate", "embedding_dim", "device", "input_pipeline"}
    assert set(parse(monkeypatch, [])) == base                        # an old command line: the old call
    kw = parse(monkeypatch, ["--input_pipeline", "device", "--hard_mining", "3"])
    assert set(kw) == base | {"hard_mining"} and kw["hard_mining"] == 3
    kw = parse(monkeypatch, ["--hard_mining", "3", "--hard_mining_genuine", "1", "--hard_mining_start", "4", "--hard_mining_every", "2"])
    assert {k: kw[k] for k in ST.MINING_FLAGS} == dict(hard_mining=3, hard_mining_genuine=1, hard_mining_start=4, hard_mining_every=2)
    capsys.readouterr()


def test_check_hard_mining():
    assert ST.check_hard_mining("host", None) is None and ST.check_hard_mining("device", None) is None
    assert ST.check_hard_mining("device", 3) == (3, 3, 2, 1)
    assert ST.check_hard_mining("device", 16, 0, 1, 5) == (16, 0, 1, 5)
    with pytest.raises(ValueError, match="--input_pipeline device"):
        ST.check_hard_mining("host", 3)
    for bad in ((0,), (17,), (3, 17), (3, -1), (3, None, 0), (3, None, 2, 0), (None, 2)):
        with pytest.raises(ValueError):
            ST.check_hard_mining("device", *bad)


def test_host_pipeline_refuses_mining(tmp_path, capsys):
    with pytest.raises(ValueError, match="hard mining needs --input_pipeline device"):
        ST.train_model(str(tmp_path), None, 1, str(tmp_path / "models"), hard_mining=2)
    with pytest.raises(ValueError, match="hard mining needs --input_pipeline device"):
        ST.main(["--data_dir", str(tmp_path), "--model_output", str(tmp_path / "models"), "--hard_mining", "2"])
    assert not (tmp_path / "models").exists()                         # refused before anything is done
    capsys.readouterr()


def test_pair_topk_host_refusals_need_no_device():
    e = torch.zeros(4, 128)
    ids = torch.zeros(4, dtype=torch.int32)
    ok = dict(e_q=e, ids_q=ids, e_r=e, ids_r=ids, k=4, same_set=True, want=("genuine", "impostor"), embedding_dim=128)
    assert SV.check_pair_topk_args(**ok) == (4, 4, ("impostor", "genuine"))
    assert SV.check_pair_topk_args(**{**ok, "want": "genuine"})[2] == ("genuine",)
    for change in (dict(k=0), dict(k=17), dict(k=1.5), dict(k=True), dict(want=()), dict(want=("best",)),
                   dict(e_r=torch.zeros(5, 128), ids_r=torch.zeros(5, dtype=torch.int32)),          # same_set with nq != nr
                   dict(e_q=torch.zeros(4, 64)), dict(e_q=e.double()), dict(ids_q=ids.long()), dict(e_q=torch.zeros(0, 128), ids_q=None)):
        with pytest.raises(ValueError):
            SV.check_pair_topk_args(**{**ok, **change})
    m = SV.SiameseNetwork(128)
    with pytest.raises(ValueError):
        m.pair_topk(e, None, e, None, 0)                              # refused before the device is looked at
    with pytest.raises(RuntimeError):
        m.eval().pair_topk(e, None, e, None, 4)                       # CPU tensors: no CPU path


def test_merge_topk_is_the_total_order():
    """The merge of a chunked same_set call, on hand-made lists with ties and padding."""
    s1, i1 = torch.tensor([[0.875, 0.5, -1.0], [0.5, 0.5, 0.25]]), torch.tensor([[4, 2, -1], [1, 3, 0]], dtype=torch.int32)
    s2, i2 = torch.tensor([[0.875, 0.75, 0.5], [-1.0, -1.0, -1.0]]), torch.tensor([[3, 9, 1], [-1, -1, -1]], dtype=torch.int32)
    s, i = SV._merge_topk([(s1, i1), (s2, i2)], 3, lowest=False)
    assert s.tolist() == [[0.875, 0.875, 0.75], [0.5, 0.5, 0.25]] and i.tolist() == [[3, 4, 9], [1, 3, 0]] and i.dtype == torch.int32
    s1, i1 = torch.tensor([[0.5, 0.875, -1.0]]), torch.tensor([[2, 4, -1]], dtype=torch.int32)
    s2, i2 = torch.tensor([[0.5, -1.0, -1.0]]), torch.tensor([[1, -1, -1]], dtype=torch.int32)
    s, i = SV._merge_topk([(s1, i1), (s2, i2)], 3, lowest=True)
    assert s.tolist() == [[0.5, 0.5, 0.875]] and i.tolist() == [[1, 2, 4]]
    s, i = SV._merge_topk([(s2, i2), (s2[:, 1:], i2[:, 1:])], 3, lowest=True)
    assert s.tolist() == [[0.5, -1.0, -1.0]] and i.tolist() == [[1, -1, -1]]


def test_library_exports_the_topk_header():
    with open(os.path.join(ROOT, "include", "siggan_verifier_topk.h")) as f:
        text = f.read()
    declared = set(re.findall(r"\bint\s+(siggan_verifier_\w+)\s*\(", text))
    assert declared == {"siggan_verifier_pairs_topk_enable", "siggan_verifier_pairs_topk"}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in siggan_verifier_topk.h but not exported"
    assert declared == set(_lib.VERIFIER_TOPK_EXPORTS)
    for older in (_lib.EXPORTS, _lib.VERIFIER_EXPORTS, _lib.VERIFIER_PAIRS_EXPORTS, _lib.VERIFIER_TRAIN_EXPORTS):
        assert not declared & set(older)
    bound = _lib.load()
    for name in declared:
        assert getattr(bound, name).argtypes is not None
    assert len(bound.siggan_verifier_pairs_topk.argtypes) == 12 and len(bound.siggan_verifier_pairs_topk_enable.argtypes) == 3
    assert int(re.search(r"#define\s+SIGGAN_PAIR_TOPK_MAX\s+(\d+)", text).group(1)) == _lib.PAIR_TOPK_MAX == 16
    body = re.search(r"typedef struct siggan_pair_topk \{(.*?)\} siggan_pair_topk;", text, re.S).group(1)
    fields = re.findall(r"\*(\w+)\s*;", body)
    assert fields == [n for n, _ in _lib.PairTopk._fields_] == ["impostor_score_dev", "impostor_index_dev", "genuine_score_dev", "genuine_index_dev"]
    lib.siggan_abi_version.restype = C.c_int
    assert lib.siggan_abi_version() == 4 == _lib.ABI_VERSION
