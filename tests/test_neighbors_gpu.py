"""siggan_knn / siggan_ball_count on the MI355X (include/siggan_neighbors.h, csrc/neighbors.hip, utils/neighbors.py), through
the C ABI and the Python wrappers.

Yardstick: numpy fp64 on the same fp32 inputs, d2 formed directly as sum_k (q_ik - r_jk)^2.  Value bound per pair, derived
and not tuned: B_ij = (dim + 4) 2^-52 (|q_i| + |r_j|)^2 -- every product of two widened fp32 values is exact; each of the
three sums of d2 = |q|^2 + |r|^2 - 2 q.r is within gamma_dim of its absolute-value sum in any order, and those are at most
|q|^2, |r|^2 and 2 |q| |r|, together (|q| + |r|)^2; three more roundings join them; the factor 2 is test_moments_gpu.py's
convention (one for each side).

Decisions -- row numbers and ball counts -- are compared exactly, and every comparison the yardstick decides by less than
2 B would have to be left out: the seeds below are chosen so that there is none (checked on the CPU when this file was
written; with normal data the gaps are about 1e-2 against bounds of about 1e-13), and a case that would leave one out fails
and says so.

Shapes are the smallest at which something can go wrong.  dim 1 (inside one K step), 4 (one step), 5 (a step and a tail),
40 (two and a half 16-feature chunks), 128 (the verifier's size); nq 1, 15, 16, 17, 67 (a partial tile, a full one, a tail,
five workgroups); nr = k, 16, 17, 131 (one wave's single tile up to nine tiles over four waves with a ragged end); k 1, 3,
16 (the list sizes 1, 4 and 16 the kernel is built for).  Two data families: standard normal rows, and unit-norm rows
where every fifth reference row is a query row plus 1e-4 noise -- the cancellation case: d2 ~ 1e-6 from terms of size 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils.neighbors import ball_count, knn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -52


def make_sets(family, dim, nq, nr, seed=0):
    rng = np.random.default_rng([seed, dim, nq, nr, 0 if family == "normal" else 1])
    q, r = rng.standard_normal((nq, dim)), rng.standard_normal((nr, dim))
    if family == "unit":
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        r /= np.linalg.norm(r, axis=1, keepdims=True)
        for j in range(0, nr, 5):                                       # every fifth reference: a near copy of a query
            r[j] = q[(j // 5) % nq] + 1e-4 * rng.standard_normal(dim)
    return q.astype(np.float32), r.astype(np.float32)


def yardstick(q, r):
    """(d2 (nq, nr), B (nq, nr)) in fp64."""
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    d2 = ((q64[:, None, :] - r64[None, :, :]) ** 2).sum(axis=2)
    nq_, nr_ = np.sqrt((q64 ** 2).sum(axis=1)), np.sqrt((r64 ** 2).sum(axis=1))
    return d2, (q.shape[1] + 4) * U * (nq_[:, None] + nr_[None, :]) ** 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_knn(got_d2, got_idx, q, r, k, exclude_self, what):
    """Row numbers exactly, values within B; fails if the yardstick cannot decide a comparison (gap <= 2 B)."""
    d2, bound = yardstick(q, r)
    if exclude_self:
        d2 = d2.copy()
        np.fill_diagonal(d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")
    rows = np.arange(q.shape[0])[:, None]
    top = order[:, :k + 1]                                               # up to the (k + 1)-th: the k-th must beat it too
    s, b = d2[rows, top], bound[rows, top]
    s = np.where(np.isinf(s), 1e200, s)                                  # the excluded diagonal: far behind everything
    gap, need = s[:, 1:] - s[:, :-1], 2 * np.maximum(b[:, 1:], b[:, :-1])
    undecided = int((gap <= need).sum())
    assert undecided == 0, f"{what}: the yardstick leaves {undecided} comparisons undecided (smallest gap / (2 x bound) {(gap / need).min():.3e}); pick another seed"
    want = order[:, :k]
    err, bnd = np.abs(got_d2 - d2[rows, want]), bound[rows, want]
    closest = float((gap / need).min()) if gap.size else float("inf")       # nr = 1: nothing to order
    print(f"{what}: worst d2 error / bound {float((err / bnd).max()):.3e}, smallest gap / (2 x bound) {closest:.3e}")
    assert got_idx.dtype == np.int32 and got_d2.dtype == np.float64 and got_idx.shape == got_d2.shape == (q.shape[0], k)
    assert np.array_equal(got_idx, want), f"{what}: row numbers differ at {np.argwhere(got_idx != want)[:4].tolist()}"
    assert (err <= bnd).all(), f"{what}: d2 off at {np.argwhere(err > bnd)[:4].tolist()}"
    assert (got_d2 >= 0).all() and (np.diff(got_d2, axis=1) >= 0).all()
    return d2, bound


def check_ball_count(q, r, what):
    """Radii between two of the yardstick's distances per ball (none, some, all queries inside), so every decision has a
    margin; counts exactly."""
    d2, bound = yardstick(q, r)
    nq, nr = d2.shape
    col = np.sort(d2, axis=0)
    radius2 = np.empty(nr)
    for j in range(nr):
        p = j % (nq + 1)                                                 # how many queries the ball holds
        radius2[j] = col[0, j] / 2 if p == 0 else col[-1, j] * 2 if p == nq else (col[p - 1, j] + col[p, j]) / 2
    margin = np.abs(d2 - radius2[None, :])
    undecided = int((margin <= 2 * bound).sum())
    assert undecided == 0, f"{what}: the yardstick leaves {undecided} ball decisions undecided; pick another seed"
    want = (d2 <= radius2[None, :]).sum(axis=1)
    got = ball_count(dev(q), dev(r), dev(radius2)).cpu().numpy()
    print(f"{what}: ball counts {int(want.min())}..{int(want.max())}, smallest margin / bound {float((margin / (2 * bound)).min()):.3e}")
    assert got.dtype == np.int32 and np.array_equal(got, want), f"{what}: counts differ at {np.argwhere(got != want)[:4].tolist()}"


CASES = [  # (dim, nq, nr, k)
    (1, 1, 1, 1), (1, 17, 16, 1), (1, 16, 131, 3), (4, 16, 17, 3), (4, 15, 17, 16), (5, 15, 131, 3), (5, 67, 16, 16),
    (40, 1, 3, 3), (40, 67, 131, 16), (40, 17, 17, 1), (128, 17, 131, 3), (128, 67, 131, 1), (128, 16, 16, 16),
]
UNIT_CASES = [(5, 15, 131, 3), (40, 67, 131, 16), (128, 17, 131, 3), (128, 67, 17, 1)]


@pytest.mark.parametrize("dim,nq,nr,k", CASES)
def test_knn_and_ball_count_normal_rows(dim, nq, nr, k):
    q, r = make_sets("normal", dim, nq, nr)
    d2, idx = knn(dev(q), dev(r), k)
    check_knn(d2.cpu().numpy(), idx.cpu().numpy(), q, r, k, False, f"normal dim={dim} nq={nq} nr={nr} k={k}")
    check_ball_count(q, r, f"normal dim={dim} nq={nq} nr={nr}")


@pytest.mark.parametrize("dim,nq,nr,k", UNIT_CASES)
def test_knn_and_ball_count_near_duplicates(dim, nq, nr, k):
    """The cancellation case: d2 ~ dim * 1e-8 out of terms of size 1 must come back within B ~ 1e-13."""
    q, r = make_sets("unit", dim, nq, nr)
    d2, idx = knn(dev(q), dev(r), k)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    yd2, bound = check_knn(d2, idx, q, r, k, False, f"unit dim={dim} nq={nq} nr={nr} k={k}")
    copies = [(((j // 5) % nq), j) for j in range(0, nr, 5)]
    near = np.array([yd2[i, j] for i, j in copies])
    assert (near < 1e-5).all() and (near > 1e-10).all() and max(bound[i, j] for i, j in copies) < 2e-13
    hit = [(i, j) for i, j in copies if idx[i, 0] == j]
    assert len(hit) >= min(len(copies), nq) // 2                         # the near copies ARE the nearest neighbours
    for i, j in hit:
        assert abs(d2[i, 0] - yd2[i, j]) <= bound[i, j] and d2[i, 0] > 0
    check_ball_count(q, r, f"unit dim={dim} nq={nq} nr={nr}")


@pytest.mark.parametrize("dim,n,k", [(5, 17, 16), (40, 4, 3), (128, 67, 3), (1, 16, 1)])
def test_exclude_diagonal(dim, n, k):
    """q = r: the row itself is absent although its d2 is 0; with nr = k + 1 every other row comes back."""
    x, _ = make_sets("normal", dim, n, 1, seed=3)
    xd = dev(x)
    d2, idx = knn(xd, xd, k, exclude_self=True)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    check_knn(d2, idx, x, x, k, True, f"exclude dim={dim} n={n} k={k}")
    assert not (idx == np.arange(n)[:, None]).any() and (d2 > 0).all()
    if n == k + 1:
        for i in range(n):
            assert sorted(idx[i].tolist()) == [j for j in range(n) if j != i]
    # without the exclusion the row itself comes first, at exactly 0.0
    kk = min(k + 1, n, _lib.KNN_MAX_K)
    d2s, idxs = knn(xd, xd, kk)
    assert np.array_equal(idxs[:, 0].cpu().numpy(), np.arange(n)) and not d2s[:, 0].cpu().numpy().any()
    assert np.array_equal(idxs[:, 1:].cpu().numpy(), idx[:, :kk - 1])
    assert np.array_equal(d2s[:, 1:].cpu().numpy(), d2[:, :kk - 1])      # the same bits with and without


@pytest.mark.parametrize("family", ["normal", "unit"])
@pytest.mark.parametrize("dim", [1, 5, 40, 128])
def test_clamp_a_row_against_itself_is_exactly_zero(family, dim):
    x, _ = make_sets(family if dim > 1 else "normal", dim, 67, 1, seed=4)
    x = x * np.float32(3.7)                                              # norms whose squares are not short numbers
    xd = dev(x)
    d2, _ = knn(xd, xd, 1)
    d2 = d2.cpu().numpy()
    assert d2.dtype == np.float64 and not d2.any() and not np.signbit(d2).any()
    # the copies at other row numbers and in other tiles: 0.0 as well
    r = np.concatenate([x[::-1], x[:3]])
    d2 = knn(xd, dev(r), 1)[0].cpu().numpy()
    assert not d2.any() and not np.signbit(d2).any()


def test_ties_come_back_lowest_row_number_first():
    rng = np.random.default_rng(5)
    dim, nr, k = 40, 70, 6
    r = rng.standard_normal((nr, dim)).astype(np.float32)
    same = [3, 17, 18, 35, 64]                                            # five tiles' worth of waves and lane groups
    for j in same[1:]:
        r[j] = r[3]
    q = rng.standard_normal((19, dim)).astype(np.float32)
    q[0] = r[3]                                                          # a five-fold tie at exactly 0
    q[1:] = r[3] + 0.05 * q[1:]                                          # the tied rows are everyone's nearest
    d2, idx = knn(dev(q), dev(r), k)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert (idx[:, :5] == np.array(same)[None, :]).all(), idx[:4].tolist()
    assert (d2[:, :5] == d2[:, :1]).all() and not d2[0, :5].any() and (d2[1:, 0] > 0).all() and (d2[:, 5] > d2[:, 4]).all()
    # all reference rows bit-identical, more of them than k, over three waves: rows 0 .. k - 1, one distance
    r = np.repeat(q[5:6], 37, axis=0)
    d2, idx = knn(dev(q), dev(r), 16)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert (idx == np.arange(16)[None, :]).all() and (d2 == d2[:, :1]).all() and d2[5, 0] == 0.0
    cnt = ball_count(dev(q), dev(r), dev(d2[3, 0] * np.ones(37))).cpu().numpy()   # a radius that IS a distance: <= holds
    assert cnt[3] == 37 and cnt[5] == 37 and set(cnt.tolist()) <= {0, 37}


def test_null_outputs():
    lib = _lib.load()
    q, r = make_sets("normal", 40, 17, 131, seed=6)
    qd, rd = dev(q), dev(r)
    d2, idx = knn(qd, rd, 3)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    only_d = torch.full((17, 3), -1.0, dtype=torch.float64, device=DEV)
    only_i = torch.full((17, 3), -1, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())                               # noqa: E731
    assert lib.siggan_knn(0, p(qd), 17, p(rd), 131, 40, 3, 0, p(only_d), None, st) == 0
    assert lib.siggan_knn(0, p(qd), 17, p(rd), 131, 40, 3, 0, None, p(only_i), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(only_d, d2) and torch.equal(only_i, idx)


def test_ball_count_zero_and_huge_radii():
    q, r = make_sets("unit", 128, 33, 131, seed=7)
    copies = {0: [4, 64, 130], 16: [5], 32: [0, 17, 18, 19]}              # query row -> its bit-identical reference rows
    for i, js in copies.items():
        r[js] = q[i]
    qd, rd = dev(q), dev(r)
    got = ball_count(qd, rd, torch.zeros(131, dtype=torch.float64, device=DEV)).cpu().numpy()
    want = np.zeros(33, np.int32)
    for i, js in copies.items():
        want[i] = len(js)
    assert np.array_equal(got, want)
    got = ball_count(qd, rd, torch.full((131,), 1e300, dtype=torch.float64, device=DEV)).cpu().numpy()
    assert (got == 131).all()
    got = ball_count(qd, rd, torch.full((131,), -1.0, dtype=torch.float64, device=DEV)).cpu().numpy()
    assert not got.any()                                                 # d2 is clamped at 0: nothing is below it


def test_invalid_arguments_launch_nothing():
    lib = _lib.load()
    q, r = make_sets("normal", 8, 5, 9, seed=8)
    qd, rd = dev(q), dev(r)
    d2 = torch.full((5, 16), -1.0, dtype=torch.float64, device=DEV)
    idx = torch.full((5, 16), -1, dtype=torch.int32, device=DEV)
    rad = torch.ones(9, dtype=torch.float64, device=DEV)
    cnt = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None    # noqa: E731

    def knn_rc(q_=qd, nq=5, r_=rd, nr=9, dim=8, k=3, excl=0, d_=d2, i_=idx):
        return lib.siggan_knn(0, p(q_), nq, p(r_), nr, dim, k, excl, p(d_), p(i_), None)

    def ball_rc(q_=qd, nq=5, r_=rd, nr=9, dim=8, rad_=rad, c_=cnt):
        return lib.siggan_ball_count(0, p(q_), nq, p(r_), nr, dim, p(rad_), p(c_), None)

    for kwargs, word in ((dict(k=0), b"k"), (dict(k=17), b"k"), (dict(k=10), b"k"), (dict(k=9, excl=1), b"k"), (dict(dim=0), b"dim"),
                         (dict(dim=1025), b"dim"), (dict(nq=0), b"nq"), (dict(nr=0), b"nr"), (dict(nq=-3), b"nq"),
                         (dict(q_=None), b"null"), (dict(r_=None), b"null"), (dict(d_=None, i_=None), b"null")):
        assert knn_rc(**kwargs) == _lib.E_ARG, kwargs
        assert word in lib.siggan_last_error(), (kwargs, lib.siggan_last_error())
    for kwargs, word in ((dict(dim=0), b"dim"), (dict(dim=1025), b"dim"), (dict(nq=0), b"nq"), (dict(nr=0), b"nr"),
                         (dict(q_=None), b"null"), (dict(r_=None), b"null"), (dict(rad_=None), b"null"), (dict(c_=None), b"null")):
        assert ball_rc(**kwargs) == _lib.E_ARG, kwargs
        assert word in lib.siggan_last_error(), (kwargs, lib.siggan_last_error())
    torch.cuda.synchronize()
    assert (d2 == -1).all() and (idx == -1).all() and (cnt == -1).all()
    assert knn_rc(k=9) == 0 and knn_rc(k=8, excl=1) == 0 and ball_rc() == 0   # the edges themselves are fine
    torch.cuda.synchronize()
    # the wrappers: argument checking in the style of FeatureMoments.update
    for bad_q, bad_r in ((qd.double(), rd), (qd, rd[:, :4]), (qd.t().contiguous().t(), rd), (qd.cpu(), rd), (qd.reshape(-1), rd),
                         (qd, rd.cpu())):
        with pytest.raises(ValueError):
            knn(bad_q, bad_r, 1)
        with pytest.raises(ValueError):
            ball_count(bad_q, bad_r, rad)
    for k in (0, 17, 10):
        with pytest.raises(ValueError):
            knn(qd, rd, k)
    with pytest.raises(ValueError):
        knn(rd, rd, 9, exclude_self=True)
    for bad in (rad.float(), rad[:8], rad.cpu(), torch.ones(18, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ball_count(qd, rd, bad)


def test_rows_that_are_not_16_byte_aligned():
    """dim % 4 == 0 but the set starts 4 bytes past an aligned address: the element-wise loader, the same bits."""
    q, r = make_sets("normal", 40, 17, 67, seed=9)
    qd, rd = dev(q), dev(r)
    off_q = torch.empty(q.size + 1, dtype=torch.float32, device=DEV)[1:].view(17, 40)
    off_r = torch.empty(r.size + 3, dtype=torch.float32, device=DEV)[3:].view(67, 40)
    off_q.copy_(qd), off_r.copy_(rd)
    assert off_q.data_ptr() % 16 == 4 and off_r.data_ptr() % 16 == 12 and off_q.is_contiguous()
    a, b = knn(qd, rd, 3), knn(off_q, off_r, 3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check_knn(b[0].cpu().numpy(), b[1].cpu().numpy(), q, r, 3, False, "unaligned dim=40")
    rad = a[0][:, 2].mean().expand(67).contiguous()
    assert torch.equal(ball_count(qd, rd, rad), ball_count(off_q, off_r, rad))


def test_determinism_stream_and_device():
    q, r = make_sets("unit", 128, 67, 131, seed=10)
    qd, rd = dev(q), dev(r)
    rad = torch.full((131,), 1.9, dtype=torch.float64, device=DEV)
    first = knn(qd, rd, 16) + (ball_count(qd, rd, rad),)
    second = knn(qd, rd, 16) + (ball_count(qd, rd, rad),)                # fresh output buffers
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert 0 < int(first[2].min()) and int(first[2].max()) < 131          # the radius cuts through the set
    # a side stream: enqueued there, nothing synchronised on the way
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(side):
        third = knn(qd, rd, 16) + (ball_count(qd, rd, rad),)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, third))
    # another current device: the call runs on the tensors' device and puts the caller's back
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            fourth = knn(qd, rd, 16) + (ball_count(qd, rd, rad),)
            assert torch.cuda.current_device() == 1
        torch.cuda.synchronize(torch.device(DEV))
        assert all(torch.equal(a, b) for a, b in zip(first, fourth))
