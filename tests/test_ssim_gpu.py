"""siggan_ssim_prepare_u8 / siggan_ssim_pairs on the MI355X (include/siggan_ssim.h, ssim.py).

Two kinds of check.  BIT CONTRACTS compare the kernel with itself and with exact constants, bitwise: x against x is 1.0f in every
mode and at every batch index, the matrix of (a, b) is the transpose of that of (b, a), PAIRED is ALL's diagonal, a pair's
value is the same in a batch of (17, 33), of (1, 1) and in SAME_SET, best / best_index are numpy's first maximum of the call's
own matrix (duplicates included; SAME_SET skips j = i), best alone is best with the matrix, a second run repeats the first, and
maps prepared in one call of n are those of n calls of 1.  ARITHMETIC compares every matrix entry with the float64 restatement
(tests/ssimcommon.py).  Its bound is not a constant: it is 16 x the largest deviation of a plain-fp32 numpy restatement from
the float64 one over the pairs scored at that size (ssimcommon.World), which measures how far an honest fp32 implementation
lands from the exact value at these images; the factor covers a legitimately different order of summation.

Sizes: one row of two windows (11, 12), (12, 12), one word beyond (16, 16), neither a multiple of a wave nor of the tile
(40, 52), (64, 64), two columns per lane (64, 128) and the two-wave workgroups of (128, 128).  Batches (1, 1), (3, 5), (17, 33)
up to 64 x 64 and (5, 7) beyond; (17, 33) is more than one workgroup of rows, more than one chunk and more than one split of
columns, and no multiple of any of them (a workgroup stages at most 8 images a side, so no larger case is needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssimcommon as SC

import signature_gan_amd  # noqa: F401
from signature_gan_amd import _lib, ssim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZE_IDS = ["x".join(map(str, s)) for s in SC.SIZES]
_SETS = {}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def bits(t):
    """The bit patterns of a device or host fp32 tensor, as int32 on the host."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return a.view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sets(h, w):
    """(World, SsimSet of A, SsimSet of B, matrix(A, B), matrix(A) in SAME_SET) -- computed once per size and left unchanged."""
    if (h, w) not in _SETS:
        world = SC.world(h, w)
        sa, sb = ssim.SsimSet(dev(world.a)), ssim.SsimSet(dev(world.b))
        _SETS[(h, w)] = (world, sa, sb, ssim.ssim_matrix(sa, sb).cpu().numpy(), ssim.ssim_matrix(sa).cpu().numpy())
    return _SETS[(h, w)]


@pytest.mark.parametrize("shape", SC.SIZES, ids=SIZE_IDS)
def test_every_entry_is_within_the_bound_of_the_float64_restatement(shape):
    world, sa, sb, ab, aa = sets(*shape)
    err_ab, err_aa = float(np.abs(ab.astype(np.float64) - world.ab64).max()), float(np.abs(aa.astype(np.float64) - world.aa64).max())
    print(f"{shape}: fp32 restatement deviates {world.fp32_deviation:.3e}, bound {world.bound:.3e}; kernel deviates {err_ab:.3e} (a, b), "
          f"{err_aa:.3e} (a, a): {max(err_ab, err_aa) / world.bound:.3f} of the bound")
    assert 1e-7 < world.fp32_deviation < 1e-4                         # the yardstick's own error is the size fp32 promises
    assert err_ab <= world.bound and err_aa <= world.bound
    for na, nb in SC.batches(*shape):                                 # and every smaller batch of the size
        got = ssim.ssim_matrix(dev(world.a[:na]), dev(world.b[:nb])).cpu().numpy()
        assert float(np.abs(got.astype(np.float64) - world.ab64[:na, :nb]).max()) <= world.bound, (na, nb)
        paired = ssim.ssim_paired(dev(world.a[:na]), dev(world.b[:na])).cpu().numpy()
        assert float(np.abs(paired.astype(np.float64) - np.diag(world.ab64)[:na]).max()) <= world.bound, (na, nb)


@pytest.mark.parametrize("shape", SC.SIZES, ids=SIZE_IDS)
def test_an_image_against_itself_is_exactly_one_in_every_mode_at_every_index(shape):
    world, sa, sb, ab, aa = sets(*shape)
    one = np.ones(world.na, np.float32)
    assert same_bits(np.diag(aa).copy(), one)                                          # SAME_SET
    assert same_bits(np.diag(ssim.ssim_matrix(sa, sa).cpu().numpy()).copy(), one)      # ALL
    assert same_bits(ssim.ssim_paired(sa, sa), one)                                    # PAIRED
    # every image of A at every index of a batch of three: rotate
    for rot in range(3):
        x = dev(np.roll(world.a[:3], rot, axis=0))
        assert same_bits(ssim.ssim_paired(x, x.clone()), np.ones(3, np.float32)), rot
    # the duplicates placed at other batch indices (ssimcommon.image_lists)
    for i, j in ((0, 1), (0, 7), (1, 2), (2, 3), (4, 6)):
        if i < world.na and j < world.nb:
            assert bits(ab[i:i + 1, j:j + 1])[0, 0] == bits(np.ones(1, np.float32))[0], (i, j)


@pytest.mark.parametrize("shape", SC.SIZES, ids=SIZE_IDS)
def test_symmetry_paired_and_batch_independence_are_bitwise(shape):
    world, sa, sb, ab, aa = sets(*shape)
    assert same_bits(ssim.ssim_matrix(sb, sa).cpu().numpy().T.copy(), ab)              # matrix(a, b)[i][j] == matrix(b, a)[j][i]
    assert same_bits(aa.T.copy(), aa)
    n = min(world.na, world.nb)
    paired = ssim.ssim_paired(dev(world.a[:n]), dev(world.b[:n]))
    assert same_bits(paired, np.diag(ab)[:n].copy())                                   # PAIRED == the diagonal of ALL
    assert same_bits(ssim.ssim_matrix(sa, sa), aa)                                     # SAME_SET == ALL on the same set
    for na, nb in SC.batches(*shape):                                                  # a pair's value in every batch it stands in
        got = ssim.ssim_matrix(dev(world.a[:na]), dev(world.b[:nb]))
        assert same_bits(got, ab[:na, :nb].copy()), (na, nb)
        assert same_bits(ssim.ssim_matrix(dev(world.a[:na])), aa[:na, :na].copy()), na
    # one pair alone, taken from the middle of both lists
    i, j = world.na - 1, world.nb - 2
    assert same_bits(ssim.ssim_matrix(dev(world.a[i:i + 1]), dev(world.b[j:j + 1])), ab[i:i + 1, j:j + 1].copy())
    # a second run gives equal bits
    assert same_bits(ssim.ssim_matrix(sa, sb), ab) and same_bits(ssim.ssim_matrix(sa), aa)


@pytest.mark.parametrize("shape", SC.SIZES, ids=SIZE_IDS)
def test_best_is_numpys_first_maximum_of_the_calls_own_matrix(shape):
    world, sa, sb, ab, aa = sets(*shape)
    for na, nb in SC.batches(*shape):
        a, b = ssim.SsimSet(dev(world.a[:na])), ssim.SsimSet(dev(world.b[:nb]))
        matrix, best, index = ssim.ssim_matrix_and_best(a, b)
        want, want_index = SC.first_maximum(matrix.cpu().numpy())
        assert same_bits(best, want) and np.array_equal(index.cpu().numpy(), want_index), (na, nb)
        alone, alone_index = ssim.ssim_best(a, b)                                      # no matrix formed: the same bits
        assert same_bits(alone, best) and torch.equal(alone_index, index), (na, nb)
        assert same_bits(matrix, ab[:na, :nb].copy())
        # SAME_SET skips j = i
        matrix, best, index = ssim.ssim_matrix_and_best(a)
        want, want_index = SC.first_maximum(matrix.cpu().numpy(), skip_diagonal=True)
        assert same_bits(best, want) and np.array_equal(index.cpu().numpy(), want_index), na
        alone, alone_index = ssim.ssim_best(a)
        assert same_bits(alone, best) and torch.equal(alone_index, index), na
        assert same_bits(matrix, aa[:na, :na].copy())
        if na == 1:
            assert best.tolist() == [-1.0] and index.tolist() == [-1]
    if world.na >= 10 and world.nb >= 8:
        # the duplicates: B[1] = B[7] = A[0] tie at 1.0 and resolve to the lower column; A[9] = A[0] find each other
        best, index = ssim.ssim_best(sa, sb)
        assert best[0].item() == 1.0 and index[0].item() == 1
        best, index = ssim.ssim_best(sa)
        assert (best[0].item(), index[0].item(), best[9].item(), index[9].item()) == (1.0, 9, 1.0, 0)
    if shape == (11, 12):
        # a tie ACROSS splits: one row against nine columns is the smallest case of two splits (columns 0..7 and 8), and above
        # B[1] and B[7] share a split.  Columns of B that are no copy of A[0], then A[0] at 3 and 8: the lower column wins
        # although the later split holds the same key value; at 8 alone: the later split's key is the only 1.0
        others = [j for j in range(world.nb) if not np.array_equal(world.b[j], world.a[0])][:9]
        for placed in ((3, 8), (8,)):
            columns = world.b[others].copy()
            columns[list(placed)] = world.a[0]
            a, b = ssim.SsimSet(dev(world.a[:1])), ssim.SsimSet(dev(columns))
            best, index = ssim.ssim_best(a, b)
            _, both, both_index = ssim.ssim_matrix_and_best(a, b)
            assert (best.item(), index.item(), both.item(), both_index.item()) == (1.0, placed[0], 1.0, placed[0]), placed


@pytest.mark.parametrize("shape", [(11, 12), (40, 52), (64, 128)], ids=["11x12", "40x52", "64x128"])
def test_maps_of_one_call_of_n_equal_n_calls_of_one(shape):
    world, sa, sb, ab, aa = sets(*shape)
    singles = torch.cat([ssim.SsimSet(dev(world.a[i:i + 1])).maps for i in range(world.na)])
    assert same_bits(singles, sa.maps) and tuple(sa.maps.shape) == (world.na, 2, shape[0] - 10, shape[1] - 10)
    assert same_bits(ssim.SsimSet(dev(world.a)).maps, sa.maps)                         # and a second run repeats it
    # plane 0 is the windowed mean, plane 1 the variance: against float64, at the scale of the values
    x = world.a.astype(np.float64)
    mu = SC._filter(x, np.float64)
    var = SC._filter(x * x, np.float64) - mu * mu
    got = sa.maps.cpu().numpy().astype(np.float64)
    assert np.abs(got[:, 0] - mu).max() <= 255.0 * 2.0 ** -20 and np.abs(got[:, 1] - var).max() <= 65025.0 * 2.0 ** -18


def raw_pairs(a, b, mode, matrix, best, index, h=None, w=None, na=None, nb=None, offset=0):
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o if t is not None else None)      # noqa: E731
    return _lib.load().siggan_ssim_pairs(0, p(a.u8), p(a.maps, offset), a.n if na is None else na, p(b.u8 if b else None),
                                         p(b.maps if b else None), (b.n if b else a.n) if nb is None else nb, a.h if h is None else h,
                                         a.w if w is None else w, mode, p(matrix), p(best), p(index),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_every_refusal_leaves_poisoned_outputs_untouched():
    world, sa, sb, ab, aa = sets(16, 16)
    matrix = torch.full((world.na, world.nb), -7.0, device=DEV)
    best = torch.full((world.na,), -7.0, device=DEV)
    index = torch.full((world.na,), -7, dtype=torch.int32, device=DEV)
    maps = torch.full_like(sa.maps, -7.0)
    cases = [dict(mode=3), dict(mode=-1), dict(h=10), dict(h=129), dict(w=8), dict(w=18), dict(w=132), dict(na=0), dict(nb=0),
             dict(offset=2), dict(mode=_lib.SSIM_PAIRED), dict(mode=_lib.SSIM_SAME_SET)]     # the last two: nb != na / a foreign b
    for kw in cases:
        kw = dict(kw)
        mode = kw.pop("mode", _lib.SSIM_ALL)
        assert raw_pairs(sa, sb, mode, matrix, best, index, **kw) == _lib.E_ARG, kw
        assert _lib.load().siggan_last_error()
    assert raw_pairs(sa, sb, _lib.SSIM_ALL, None, None, None) == _lib.E_ARG                        # no output
    assert raw_pairs(sa, sa, _lib.SSIM_PAIRED, matrix, best, None) == _lib.E_ARG                   # best in PAIRED
    assert raw_pairs(sa, sa, _lib.SSIM_PAIRED, matrix, None, index) == _lib.E_ARG
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    u8 = dev(world.a)
    prepare = _lib.load().siggan_ssim_prepare_u8
    for n, h, w, off in ((0, 16, 16, 0), (3, 10, 16, 0), (3, 16, 10, 0), (3, 16, 132, 0), (3, 129, 16, 0), (3, 16, 16, 1)):
        assert prepare(0, C.c_void_p(u8.data_ptr()), n, h, w, C.c_void_p(maps.data_ptr() + off), stream) == _lib.E_ARG, (n, h, w, off)
    assert prepare(0, None, 3, 16, 16, C.c_void_p(maps.data_ptr()), stream) == _lib.E_ARG
    torch.cuda.synchronize()
    assert (matrix == -7.0).all() and (best == -7.0).all() and (index == -7).all() and (maps == -7.0).all()
    # the Python layer refuses before it touches the library, in the order type, dtype, rank, sizes, device, layout
    x = dev(world.a)
    for bad, word in ((world.a, "tensor"), (x.float(), "uint8"), (x[0], "N, H, W"), (x[:0], "no image"), (x[:, :10], "height"),
                      (x[:, :, :10], "width"), (x.cpu(), "no CPU path"), (x[:, :, :12], "contiguous")):
        for call in (lambda: ssim.SsimSet(bad), lambda: ssim.ssim_matrix(bad, x), lambda: ssim.ssim_best(x, bad),
                     lambda: ssim.ssim_paired(x, bad)):
            with pytest.raises(ValueError, match=word):
                call()
    with pytest.raises(ValueError, match="equal size"):
        ssim.ssim_matrix(sa, sets(12, 12)[1])
    with pytest.raises(ValueError, match="equally many"):
        ssim.ssim_paired(sa, sb)
