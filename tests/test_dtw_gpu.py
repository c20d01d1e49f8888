"""siggan_dtw_profiles_u8 / siggan_dtw_pairs on the MI355X (include/siggan_dtw.h, dtw.py).

Everything is integer arithmetic, so every comparison is exact equality: the profiles and every matrix entry against the numpy
restatement (tests/dtwcommon.py), the kernel against itself (symmetry, PAIRED against ALL's diagonal, best against the matrix, a
pair's value at any place in the launch), and the closed-form extremes that 16-bit sums or a leaking sentinel would miss.

Widths: 4, 12, 64 (one full array of lanes), 68 (the first that needs a second strip of rows) and 128 (two full strips).  Bands 0,
1, default_band(w) and w - 1.  Set sizes (5, 7), (1, 1) and (3, 70): the last gives one wave several columns in a row and more
than one split of columns.  The yardstick matrices are computed once per (size, band) over the longest lists; the smaller cases
are prefixes."""
import ctypes as C

import numpy as np
import pytest
import torch

import dtwcommon as DC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, dtw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE_IDS = ["x".join(map(str, s)) for s in DC.SIZES]
_SETS = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.cpu().numpy()


def sets(h, w):
    """(World, DtwSet of A, DtwSet of B) -- made once per size and left unchanged."""
    if (h, w) not in _SETS:
        world = DC.world(h, w)
        _SETS[(h, w)] = (world, dtw.DtwSet(dev(world.a)), dtw.DtwSet(dev(world.b)))
    return _SETS[(h, w)]


def profile_images(h, w):
    """The contents of the issue at this size: paper, ink, empty columns between inked ones, every second row, single pixels in
    the first and the last row, and two of the world's images; bytes on both sides of every threshold tried."""
    paper, inked = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    gaps = np.full((h, w), 255, np.uint8)
    gaps[:, 0::3] = 0
    rows = np.full((h, w), 255, np.uint8)
    rows[0::2] = 0
    corners = np.full((h, w), 255, np.uint8)
    corners[0, 0] = corners[h - 1, w - 1] = corners[0, w // 2] = corners[h - 1, 1] = 0
    levels = np.random.default_rng(h * 131 + w).choice(np.array([0, 1, 127, 128, 129, 254, 255], np.uint8), (h, w))
    world = DC.world(h, w)
    return np.stack([paper, inked, gaps, rows, corners, levels, world.a[0], world.a[3]])


@pytest.mark.parametrize("shape", DC.SIZES, ids=SIZE_IDS)
def test_profiles_equal_the_restatement(shape):
    h, w = shape
    images = profile_images(h, w)
    x = dev(images)
    for threshold in (1, 128, 255):
        got = dtw.column_profiles(x, threshold)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(images), w, 4)
        assert np.array_equal(host(got), DC.profiles(images, threshold)), threshold
        assert torch.equal(dtw.DtwSet(x, threshold).profiles, got)
    assert torch.equal(dtw.column_profiles(x[:, None]), dtw.column_profiles(x))        # (N, 1, H, W) is the same bytes
    if (h, w) == (128, 128):
        assert host(dtw.column_profiles(x))[3, 0].tolist() == [64, 0, 126, 64]         # every second row: r = 64


@pytest.mark.parametrize("shape", DC.SIZES, ids=SIZE_IDS)
def test_every_entry_equals_the_restatement(shape):
    world, sa, sb = sets(*shape)
    for band in DC.bands(world.w):
        want = world.ab(band)
        for na, nb in DC.BATCHES:
            got = dtw.dtw_matrix(dev(world.a[:na]), dev(world.b[:nb]), band)
            assert got.dtype == torch.int32 and tuple(got.shape) == (na, nb)
            assert np.array_equal(host(got), want[:na, :nb]), (band, na, nb)
        assert np.array_equal(host(dtw.dtw_matrix(sa, band=band)), world.aa(band)), band
    assert np.array_equal(host(dtw.dtw_matrix(sa, sb)), world.ab(DC.default_band(world.w)))   # band None is the default band


def test_the_extremes_are_exact():
    x = dtw.DtwSet(dev(DC.extreme_images()))
    for band in (0, 16, 127):
        assert np.array_equal(host(dtw.dtw_matrix(x, band=band)), DC.EXTREMES), band
        assert np.array_equal(host(dtw.dtw_matrix(x, x, band)), DC.EXTREMES), band
        assert host(dtw.dtw_paired(x, dtw.DtwSet(dev(DC.extreme_images()[[1, 0, 0]])), band)).tolist() == [32768, 32768, 16384]


@pytest.mark.parametrize("shape", DC.SIZES, ids=SIZE_IDS)
def test_the_kernel_agrees_with_itself(shape):
    world, sa, sb = sets(*shape)
    for band in DC.bands(world.w):
        aa = dtw.dtw_matrix(sa, band=band)
        assert not aa.diagonal().any() and torch.equal(aa, aa.T.contiguous())
        ab, ba = dtw.dtw_matrix(sa, sb, band), dtw.dtw_matrix(sb, sa, band)
        assert torch.equal(ab, ba.T.contiguous())
        n = min(sa.n, sb.n)
        assert torch.equal(dtw.dtw_paired(sa, sb.first(n), band), ab.diagonal()[:n].contiguous())
        matrix, best, index = dtw.dtw_matrix_and_best(sa, sb, band)
        alone, alone_index = dtw.dtw_best(sa, sb, band)
        assert torch.equal(matrix, ab) and torch.equal(best, alone) and torch.equal(index, alone_index)
        matrix, best, index = dtw.dtw_matrix_and_best(sa, band=band)
        alone, alone_index = dtw.dtw_best(sa, band=band)
        assert torch.equal(matrix, aa) and torch.equal(best, alone) and torch.equal(index, alone_index)
        assert torch.equal(dtw.dtw_matrix(sa, sb, band), ab)                           # a second run repeats the first


@pytest.mark.parametrize("shape", [(64, 64), (33, 68), (128, 128)], ids=["64x64", "33x68", "128x128"])
def test_a_pairs_value_does_not_depend_on_its_place_in_the_launch(shape):
    world, sa, sb = sets(*shape)
    rng = np.random.default_rng(shape[1])
    for band in (1, DC.default_band(world.w)):
        whole = dtw.dtw_matrix(sa, sb, band)
        for _ in range(2):
            p, q = rng.permutation(world.a.shape[0]), rng.permutation(world.b.shape[0])
            got = dtw.dtw_matrix(dev(world.a[p]), dev(world.b[q]), band)
            assert torch.equal(got, whole[dev(p)][:, dev(q)]), band
        part = dtw.dtw_matrix(dev(world.a[3:4]), dev(world.b[40:43]), band)             # and in a launch of its own
        assert torch.equal(part, whole[3:4, 40:43])


@pytest.mark.parametrize("shape", DC.SIZES, ids=SIZE_IDS)
def test_best_is_the_first_minimum(shape):
    world, sa, sb = sets(*shape)
    for band in (0, DC.default_band(world.w)):
        for na, nb in DC.BATCHES:
            best, index = dtw.dtw_best(sa.first(na), sb.first(nb), band)
            want, want_index = DC.first_minimum(world.ab(band)[:na, :nb])
            assert best.dtype == index.dtype == torch.int32
            assert np.array_equal(host(best), want) and np.array_equal(host(index), want_index), (band, na, nb)
        for na in (5, 3, 1):
            best, index = dtw.dtw_best(sa.first(na), band=band)                        # SAME_SET skips j = i
            want, want_index = DC.first_minimum(world.aa(band)[:na, :na], skip_diagonal=True)
            assert np.array_equal(host(best), want) and np.array_equal(host(index), want_index), (band, na)
            if na == 1:
                assert best.tolist() == [-1] and index.tolist() == [-1]


def test_ties_go_to_the_lower_index_and_same_set_skips_itself():
    world, sa, sb = sets(64, 64)
    # B[1] = B[4] = B[9] = A[0]; B[2] is A[1] (paper), B[3] is A[2] (ink): ties at 0 resolve to the lower column
    best, index = dtw.dtw_best(sa, sb)
    assert best[:3].tolist() == [0, 0, 0] and index[:3].tolist() == [1, 2, 3]
    best, index = dtw.dtw_best(sa, dtw.DtwSet(dev(world.b[[4, 9, 1, 0]])))
    assert (best[0].item(), index[0].item()) == (0, 0)
    # a duplicate of a_i elsewhere in the same set gives 0 at that index, not at i
    twice = dtw.DtwSet(dev(np.concatenate([world.a, world.a[[3, 0]]])))
    best, index = dtw.dtw_best(twice)
    assert (best[0].item(), index[0].item(), best[6].item(), index[6].item()) == (0, 6, 0, 0)
    assert (best[3].item(), index[3].item(), best[5].item(), index[5].item()) == (0, 5, 0, 3)
    assert best[1].item() > 0 and index[1].item() != 1


def test_a_non_default_stream_a_slice_and_two_heights():
    world, sa, sb = sets(64, 64)
    want = dtw.dtw_matrix(sa, sb)
    side = torch.cuda.Stream(device=DEV)
    x, y = dev(world.a), dev(world.b)
    with torch.cuda.stream(side):
        on_side = dtw.dtw_matrix_and_best(x, y)
    side.synchronize()
    assert torch.equal(on_side[0], want) and torch.equal(on_side[1], dtw.dtw_best(sa, sb)[0])
    # a 4-byte-aligned slice of a larger tensor
    big = torch.full((world.b.shape[0] + 3, 64, 64), 9, dtype=torch.uint8, device=DEV)
    big[2:-1] = y
    assert big[2:-1].data_ptr() % 4 == 0 and big[2:-1].data_ptr() != big.data_ptr()
    assert torch.equal(dtw.dtw_matrix(x, big[2:-1]), want)
    # sets of different heights and equal width: rows are absolute
    small = DC.world(33, 68)
    tall = np.full((small.b.shape[0], 50, 68), 255, np.uint8)
    tall[:, :33] = small.b
    sa68, tall68 = dtw.DtwSet(dev(small.a)), dtw.DtwSet(dev(tall))
    assert (sa68.h, tall68.h, sa68.w, tall68.w) == (33, 50, 68, 68)
    for band in (0, 8):
        assert np.array_equal(host(dtw.dtw_matrix(sa68, tall68, band)), DC.dtw_matrix(small.pa, DC.profiles(tall), band))
    with pytest.raises(ValueError, match="equal width"):
        dtw.dtw_matrix(sa, sa68)


def raw_pairs(a, b, mode, matrix, best, index, w=None, band=2, na=None, nb=None, offset=0):
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o if t is not None else None)        # noqa: E731
    return _lib.load().siggan_dtw_pairs(0, p(a.profiles, offset), a.n if na is None else na, p(b.profiles if b else None),
                                        (b.n if b else a.n) if nb is None else nb, a.w if w is None else w, band, mode, p(matrix),
                                        p(best), p(index), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_every_refusal_leaves_poisoned_outputs_untouched():
    world, sa, sb = sets(7, 12)
    matrix = torch.full((sa.n, sb.n), -7, dtype=torch.int32, device=DEV)
    best = torch.full((sa.n,), -7, dtype=torch.int32, device=DEV)
    index = torch.full((sa.n,), -7, dtype=torch.int32, device=DEV)
    prof = torch.full_like(sa.profiles, 249)
    cases = [dict(mode=3), dict(mode=-1), dict(w=0), dict(w=10), dict(w=132), dict(band=-1), dict(band=12), dict(na=0), dict(nb=0),
             dict(offset=2), dict(mode=_lib.DTW_PAIRED), dict(mode=_lib.DTW_SAME_SET)]       # the last two: nb != na / a foreign b
    for kw in cases:
        kw = dict(kw)
        mode = kw.pop("mode", _lib.DTW_ALL)
        assert raw_pairs(sa, sb, mode, matrix, best, index, **kw) < 0, kw
        assert _lib.load().siggan_last_error()
    assert raw_pairs(sa, sb, _lib.DTW_ALL, None, None, None) == _lib.E_ARG                          # no output pointer
    assert b"no output" in _lib.load().siggan_last_error()
    assert raw_pairs(sa, sa, _lib.DTW_PAIRED, matrix, best, None) == _lib.E_ARG                     # best in PAIRED
    assert b"PAIRED" in _lib.load().siggan_last_error()
    assert raw_pairs(sa, sa, _lib.DTW_PAIRED, matrix, None, index) == _lib.E_ARG
    assert raw_pairs(sa, sb, _lib.DTW_ALL, matrix, best, index, offset=2) == _lib.E_ARG             # an unaligned pointer
    assert b"aligned" in _lib.load().siggan_last_error()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u8 = dev(world.a)
    profiles = _lib.load().siggan_dtw_profiles_u8
    for n, h, w, thr, off in ((0, 7, 12, 128, 0), (5, 0, 12, 128, 0), (5, 129, 12, 128, 0), (5, 7, 10, 128, 0), (5, 7, 132, 128, 0),
                              (5, 7, 12, 0, 0), (5, 7, 12, 256, 0), (5, 7, 12, 128, 2)):
        assert profiles(0, C.c_void_p(u8.data_ptr()), n, h, w, thr, C.c_void_p(prof.data_ptr() + off), stream) == _lib.E_ARG, (n, h, w, thr, off)
    assert profiles(0, None, 5, 7, 12, 128, C.c_void_p(prof.data_ptr()), stream) == _lib.E_ARG
    assert profiles(0, C.c_void_p(u8.data_ptr()), 5, 7, 12, 128, None, stream) == _lib.E_ARG
    torch.cuda.synchronize()
    assert (matrix == -7).all() and (best == -7).all() and (index == -7).all() and (prof == 249).all()
    # the Python layer's layout refusal needs a device tensor: it comes last
    x = dev(DC.world(64, 64).a)
    for call in (lambda: dtw.DtwSet(x[:, :, :12]), lambda: dtw.dtw_matrix(x, x.transpose(1, 2)),
                 lambda: dtw.column_profiles(x[:, :, 4:16])):
        with pytest.raises(ValueError, match="contiguous"):
            call()
    with pytest.raises(ValueError, match="no CPU path"):
        dtw.dtw_matrix(x, x.cpu())


def test_a_shifted_copy_finds_its_original_only_with_a_band():
    originals = DC.signature_family(64, 64, 12)
    moved = DC.shifted(originals, 3)
    po, pm = DC.profiles(originals), DC.profiles(moved)
    want_elastic, want_rigid = DC.first_minimum(DC.dtw_matrix(pm, po, 8)), DC.first_minimum(DC.dtw_matrix(pm, po, 0))
    found_elastic, found_rigid = int((want_elastic[1] == np.arange(12)).sum()), int((want_rigid[1] == np.arange(12)).sum())
    print(f"the restatement: {found_elastic} of 12 moved copies find their original at band 8, {found_rigid} at band 0")
    assert found_elastic == 12 and found_rigid < 12
    so, sm = dtw.DtwSet(dev(originals)), dtw.DtwSet(dev(moved))
    best, index = dtw.dtw_best(sm, so, 8)
    assert np.array_equal(host(index), np.arange(12)) and np.array_equal(host(best), want_elastic[0])
    best, index = dtw.dtw_best(sm, so, 0)
    assert int((host(index) == np.arange(12)).sum()) == found_rigid < 12
    assert np.array_equal(host(index), want_rigid[1]) and np.array_equal(host(best), want_rigid[0])
