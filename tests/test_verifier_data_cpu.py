"""Verifier trainer's input pipeline, CPU side: the new symbol sits in its own header and export table, the pair plan
(order + every draw + what is left of torch's global generator) is pinned against the real torch DataLoader, and the host's
kernel parameters against Pillow itself through a numpy emulation of the kernel contract.  tests/test_verifier_data_gpu.py
checks the kernel and the loader."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import verifierdatacommon as DC

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_train as ST
from signature_gan_amd import verifier_data as VD


def test_library_exports_the_data_header():
    with open(os.path.join(DC.ROOT, "include", "siggan_verifier_data.h")) as f:
        declared = set(re.findall(r"\b(?:int|int64_t)\s+(siggan_\w+)\s*\(", f.read()))
    assert declared == {"siggan_pairs_augment"}
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "siggan_pairs_augment"), "declared in siggan_verifier_data.h but not exported"
    assert _lib.VERIFIER_DATA_EXPORTS == ("siggan_pairs_augment",)
    for older in (_lib.EXPORTS, _lib.VERIFIER_EXPORTS, _lib.VERIFIER_TRAIN_EXPORTS):
        assert "siggan_pairs_augment" not in older
    for header in ("siggan.h", "siggan_mlp.h", "siggan_verifier.h", "siggan_verifier_train.h"):
        with open(os.path.join(DC.ROOT, "include", header)) as f:
            assert not re.search(r"siggan_pairs_augment\s*\(", f.read()), header
    lib.siggan_abi_version.restype = C.c_int
    assert lib.siggan_abi_version() == 4                  # a symbol only added
    assert _lib.load().siggan_pairs_augment.argtypes is not None


class _PairDraws(torch.utils.data.Dataset):
    """What one item of the reference's pair dataset draws from torch's global generator with the train transform
    (torchvision's RandomAffine.get_params, then RandomHorizontalFlip), without the images."""

    def __init__(self, n, augment):
        self.n, self.augment = n, augment

    def __len__(self):
        return self.n

    @staticmethod
    def _image():
        angle = float(torch.empty(1).uniform_(-5.0, 5.0).item())
        tx = int(round(torch.empty(1).uniform_(-6.4, 6.4).item()))
        ty = int(round(torch.empty(1).uniform_(-6.4, 6.4).item()))
        scale = float(torch.empty(1).uniform_(0.9, 1.1).item())
        flip = bool(torch.rand(1) < 0.1)
        return [angle, float(tx), float(ty), scale, float(flip)]

    def __getitem__(self, i):
        d = self._image() + self._image() if self.augment else []
        return torch.tensor([float(i)] + d, dtype=torch.float64)


def _same(ref, plan):
    batches, draws = plan
    assert [len(b) for b in batches] == [r.shape[0] for r in ref]
    pos = 0
    for b, r in zip(batches, ref):
        m = len(b)
        assert b == [int(v) for v in r[:, 0]]
        if draws is None:
            assert r.shape[1] == 1
        else:
            for j in range(2):
                for c, key in enumerate(("angle", "tx", "ty", "scale", "flip")):
                    assert np.array_equal(draws[key][pos:pos + m, j].astype(np.float64), r[:, 1 + 5 * j + c].numpy()), (key, j)
        pos += m
    if draws is not None:
        assert all(v.shape == (pos, 2) for v in draws.values())


@pytest.mark.parametrize("shuffle,drop_last", [(True, False), (False, False), (True, True)])
def test_pair_plan_is_the_dataloaders(shuffle, drop_last):
    n, bs = 13, 5                                         # batches of 5, 5 and 3 (5, 5 with drop_last)
    DL = torch.utils.data.DataLoader
    train = DL(_PairDraws(n, True), batch_size=bs, shuffle=shuffle, num_workers=0, drop_last=drop_last)
    val = DL(_PairDraws(4, False), batch_size=bs, shuffle=False, num_workers=0)
    torch.manual_seed(77)
    ref = [[b.clone() for b in train], [b.clone() for b in val], [b.clone() for b in train]]
    ref_next = torch.rand(1)
    torch.manual_seed(77)
    plans = [VD.plan_pair_epoch(n, bs, shuffle, drop_last), VD.plan_pair_epoch(4, bs, False, augment=False),
             VD.plan_pair_epoch(n, bs, shuffle, drop_last)]
    next_ = torch.rand(1)
    assert len(ref[0]) == (2 if drop_last else 3)
    for r, p in zip(ref, plans):
        _same(r, p)
    assert plans[1][1] is None
    assert torch.equal(ref_next, next_), "the plan leaves torch's global generator elsewhere than the DataLoader does"
    if shuffle:
        assert plans[0][0] != plans[2][0]
        assert drop_last or sorted(i for b in plans[0][0] for i in b) == list(range(n))
    assert not np.array_equal(plans[0][1]["angle"], plans[2][1]["angle"])


def test_flips_and_rounding_occur():
    """The plan's rare branches are really drawn: some flips at p = 0.1, every translation in -6..6."""
    torch.manual_seed(5)
    _, d = VD.plan_pair_epoch(400, 32, True)
    assert 0.05 < d["flip"].mean() < 0.15
    assert set(np.unique(d["tx"])) == set(range(-6, 7)) == set(np.unique(d["ty"]))
    assert d["angle"].min() >= -5 and d["angle"].max() <= 5 and d["scale"].min() >= np.float32(0.9) and d["scale"].max() <= np.float32(1.1)


FORCED = ([(0.0, 0, 0, 1.0)] + [(0.0, tx, ty, 1.0) for tx in (6, -6) for ty in (6, -6)] + [(0.0, 6, 0, 0.9), (0.0, 0, -6, 1.1)] +
          [(a, 0, 0, s) for a in (5.0, -5.0) for s in (0.9, 1.1)] + [(1e-9, 0, 0, 1.0), (1e-9, -6, 6, 1.1)])


def test_host_parameters_reproduce_pillow():
    rng = np.random.default_rng(11)
    n = 200
    angle = rng.uniform(-5, 5, n).astype(np.float32).astype(np.float64)
    tx, ty = rng.integers(-6, 7, n), rng.integers(-6, 7, n)
    scale = rng.uniform(0.9, 1.1, n).astype(np.float32).astype(np.float64)
    flip = rng.random(n) < 0.5
    forced = [c + (f,) for c in FORCED for f in (False, True)]
    angle = np.concatenate([angle, [c[0] for c in forced]])
    tx, ty = np.concatenate([tx, [c[1] for c in forced]]), np.concatenate([ty, [c[2] for c in forced]])
    scale = np.concatenate([scale, [c[3] for c in forced]])
    flip = np.concatenate([flip, [c[4] for c in forced]])
    prm, tab = VD.build_pair_params(angle, tx, ty, scale, flip)
    total = n + len(forced)
    assert prm.shape == (total, 8) and prm.dtype == np.int32 and tab.shape == (total, 2, 64) and tab.dtype == np.int16
    assert (prm[angle == 0, 0] == 2).all() and (prm[angle != 0, 0] == 1).all()      # Pillow's own path choice
    assert np.array_equal(prm[:, 7] & 1, flip.astype(np.int32))
    for i in range(total):
        img = rng.integers(0, 256, (64, 64), dtype=np.uint8)
        want = DC.pil_affine(img, angle[i], tx[i], ty[i], scale[i], flip[i])
        assert np.array_equal(DC.emulate(img, prm[i], tab[i]), want), (i, angle[i], tx[i], ty[i], scale[i], flip[i])
    ident = n                                             # identity: every pixel its own source
    assert np.array_equal(tab[ident, 0], np.arange(64)) and np.array_equal(tab[ident, 1], np.arange(64))


def test_matrix_is_the_oracles():
    for a, tx, ty, s in FORCED + [(3.25, 5, -2, 1.03)]:
        assert VD.inverse_affine_matrix(a, tx, ty, s) == DC.A.tv_inverse_affine_matrix([32.0, 32.0], a, [tx, ty], s, [0.0, 0.0])


def test_no_cpu_route_and_flag_values():
    class _Empty:
        pairs = []
    with pytest.raises(RuntimeError, match="ROCm"):
        VD.DevicePairLoader(_Empty(), 4, False, False, device="cpu")
    with pytest.raises(ValueError, match="input_pipeline"):
        ST.train_model("nowhere", None, 1, "nowhere", input_pipeline="gpu")
    with pytest.raises(SystemExit):
        ST.main(["--data_dir", "x", "--input_pipeline", "gpu"])


def test_argument_errors_are_refused_before_any_device_call():
    lib = _lib.load()
    ok = dict(cache=4096, n_images=1, index=4096, out=4096, n=2, size=64, fill=0)      # never dereferenced: every case is refused
    for change, text in ((dict(size=128), "size"), (dict(n=0), "n must"), (dict(cache=None), "null"), (dict(out=4098), "aligned"),
                         (dict(n_images=0), "empty"), (dict(fill=256), "fill")):
        a = {**ok, **change}
        rc = lib.siggan_pairs_augment(0, a["cache"], a["n_images"], a["index"], None, None, a["out"], a["n"], a["size"], a["fill"], None)
        assert rc == _lib.E_ARG and text in lib.siggan_last_error().decode(), change
