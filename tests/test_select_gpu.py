"""siggan_select_topk / siggan_gather_u8 (Engine.select_topk / gather_u8): the ranking and gathering that end
realism-filtered generation.  The expected order is Python's own stable sort, sorted(range(m), key=s.__getitem__,
reverse=True)[:k] on the float32 scores; the expected gather is numpy fancy indexing."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _scores(name):
    rng = np.random.default_rng(20)
    if name == "one":
        return np.array([0.25], np.float32), 1
    if name == "five":                                      # the issue's example first: ties keep ascending index order
        return np.array([.5, 1, .5, 1, .2], np.float32), 5
    if name == "issue":
        return np.array([.5, 1, .5, 1, .2, 1], np.float32), 6
    if name == "m257":                                      # one score past a block of 256 threads
        return rng.random(257, dtype=np.float32), 100
    if name == "ties1000":                                  # 7 distinct values: heavy ties, every rank kept
        return rng.choice(np.array([0.0, 0.1, 0.25, 0.5, 0.75, 0.999, 1.0], np.float32), size=1000), 1000
    if name == "zeros":                                     # -0.0 == 0.0, a saturated 1.0 repeated, subnormals ordered by value
        tiny = np.array([1e-45, 3e-45, 1e-40, -1e-45, -1e-40, 1.1754942e-38], np.float32)
        assert (tiny != 0).all()
        base = np.concatenate([np.array([-0.0, 0.0, 1.0, 0.0, 1.0, -0.0, 1.0, -1.0, 0.5], np.float32), tiny, tiny[::-1]])
        return np.concatenate([base, base[::-1]]), 2 * len(base)
    if name == "m4099":                                     # three LDS tiles of 2048, the last one ragged and no multiple of 4
        s = rng.random(4099, dtype=np.float32)
        s[[0, 2047, 2048, 4095, 4096, 4098]] = 2.0          # ties across the tile borders, at both ends
        return s, 64
    raise KeyError(name)


def _want(s, k):
    v = [float(x) for x in s]
    return sorted(range(len(v)), key=v.__getitem__, reverse=True)[:k]


@pytest.mark.parametrize("name", ["one", "five", "issue", "m257", "ties1000", "zeros", "m4099"])
def test_topk_is_pythons_stable_sort(name):
    from signature_gan_amd import _lib
    from signature_gan_amd.engine import Engine
    s, k = _scores(name)
    dev = torch.from_numpy(s).cuda()
    got = Engine.select_topk(dev, k)
    assert got.dtype == torch.int32 and tuple(got.shape) == (k,)
    assert got.cpu().tolist() == _want(s, k)
    if name == "issue":
        assert got.cpu().tolist() == [1, 3, 5, 0, 2, 4]
    assert torch.equal(Engine.select_topk(dev, k), got)                   # equal input, equal output
    if k > 1:                                                             # a shorter selection is a prefix, the rest untouched
        buf = torch.full((k,), -5, dtype=torch.int32, device="cuda")
        rc = _lib.load().siggan_select_topk(0, C.c_void_p(dev.data_ptr()), len(s), k // 2, C.c_void_p(buf.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == 0 and buf.cpu().tolist() == _want(s, k // 2) + [-5] * (k - k // 2)


def test_topk_at_the_cap_selects_across_every_tile():
    from signature_gan_amd.engine import Engine
    m, k = 65536, 300
    s = np.random.default_rng(21).integers(0, 512, size=m).astype(np.float32) / 512                # ~128 of each value
    got = Engine.select_topk(torch.from_numpy(s).cuda(), k).cpu().tolist()
    assert got == _want(s, k)


@pytest.mark.parametrize("binarize", [None, 127, 1, 0, 255])
def test_gather_is_fancy_indexing(binarize):
    from signature_gan_amd.engine import Engine
    from signature_gan_amd.utils.inference import binarize_uint8
    rng = np.random.default_rng(22)
    pool = rng.integers(0, 256, size=(9, 64, 64), dtype=np.uint8)         # 4096 pixels
    pool[3] = np.resize(np.arange(256, dtype=np.uint8), (64, 64))
    index = np.array([8, 3, 3, 0, 5], np.int32)
    got = Engine.gather_u8(torch.from_numpy(pool).cuda(), torch.from_numpy(index).cuda(), binarize=binarize)
    want = pool[index] if binarize is None else binarize_uint8(pool[index], binarize)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 64, 64)
    assert np.array_equal(got.cpu().numpy(), want)


def test_gather_small_rows_and_stray_indices():
    from signature_gan_amd.engine import Engine
    pool = np.arange(7 * 12, dtype=np.uint8).reshape(7, 12)               # three words per row: less than one block
    got = Engine.gather_u8(torch.from_numpy(pool).cuda(), torch.tensor([6, 0], dtype=torch.int32, device="cuda"))
    assert np.array_equal(got.cpu().numpy(), pool[[6, 0]])
    # an index outside the pool reads nothing and leaves its row unwritten
    from signature_gan_amd import _lib
    out = torch.full((3, 12), 9, dtype=torch.uint8, device="cuda")
    idx = torch.tensor([7, 2, -1], dtype=torch.int32, device="cuda")
    dpool = torch.from_numpy(pool).cuda()
    rc = _lib.load().siggan_gather_u8(0, C.c_void_p(dpool.data_ptr()), 7, 12, C.c_void_p(idx.data_ptr()), 3, -1,
                                      C.c_void_p(out.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out.cpu().numpy(), np.stack([np.full(12, 9, np.uint8), pool[2], np.full(12, 9, np.uint8)]))


def test_refusals():
    from signature_gan_amd import _lib
    from signature_gan_amd.engine import Engine
    s = torch.rand(8, device="cuda")
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            Engine.select_topk(s, k)
    lib = _lib.load()
    big = torch.zeros(65537, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert lib.siggan_select_topk(0, C.c_void_p(big.data_ptr()), 65537, 4, C.c_void_p(idx.data_ptr()), None) == -1     # m > 65536
    assert lib.siggan_select_topk(0, C.c_void_p(big.data_ptr()), 65536, 4, C.c_void_p(idx.data_ptr()), None) == 0
    assert lib.siggan_select_topk(0, C.c_void_p(big.data_ptr()), 0, 0, C.c_void_p(idx.data_ptr()), None) == -1
    with pytest.raises(ValueError):
        Engine.select_topk(s.double(), 2)
    pool = torch.zeros(4, 10, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):                                       # pixels % 4 != 0
        Engine.gather_u8(pool, idx[:2])
    pool = torch.zeros(4, 16, dtype=torch.uint8, device="cuda")
    for bad in (256, -1):
        with pytest.raises(ValueError):
            Engine.gather_u8(pool, idx[:2], binarize=bad)
    with pytest.raises(ValueError):
        Engine.gather_u8(pool, idx[:2].long())
    with pytest.raises(ValueError):                                       # k = 0
        Engine.gather_u8(pool, idx[:0])
    torch.cuda.synchronize()
