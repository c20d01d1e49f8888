"""The yardstick of diverse selection (include/siggan_diverse.h): the header's semantics restated line for line in numpy
fp64, the error bound of one squared distance, and the input families the CPU and GPU tests share.

Bound.  d2 = sum_k (x_ik - x_pk)^2 over fp32 values widened to fp64.  Each difference is exact or within one rounding, each
square is one rounding, and the dim terms meet in dim - 1 additions whatever the summation tree (an addition of 0.0 is
exact), so any fp64 evaluation is within (dim + 1) * 2^-53 * d2 (1 + o(1)) of the exact sum; the yardstick is such an
evaluation too, so two of them differ by at most twice that: B = (dim + 4) * 2^-52 * d2 -- the factor 2 between a value's
own error and the distance of two evaluations is the convention of tests/test_moments_gpu.py.  The bound is derived, not tuned.

A pick is "undecided" when the best and the second-best candidate value are closer than 2 B (B of the larger): another
summation order may then choose the other row, and order[] of two correct implementations may differ from there on."""
import numpy as np

EPS = 2.0 ** -52


def bound(d2, dim):
    """B for a value d2 (an array or a number); 0 for +inf (never compared by tolerance) and for an exact 0."""
    d2 = np.asarray(d2, dtype=np.float64)
    return np.where(np.isfinite(d2), (dim + 4) * EPS * d2, 0.0)


def d2_to_row(x64, p):
    return ((x64 - x64[p]) ** 2).sum(1)


def select(x, n_select, eligible=None, anchor_d2=None, first=-1, min_gain2=0.0):
    """(order int32 (n_select,), gain2 fp64 (n_select,), count, min_d2 fp64 (n,), gap fp64 (n_select,), undecided bool
    (n_select,)): the semantics of siggan_select_diverse.  gap[t]: the best minus the second-best candidate value at pick t
    (+inf where there was no second candidate, the pick was forced, or both are +inf -- a tie the row number decides in every
    implementation); undecided[t]: gap[t] < 2 B of the best value (but see the note on dim = 1 in the loop)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, dim = x64.shape
    elig = np.ones(n, bool) if eligible is None else np.asarray(eligible).astype(bool)
    m = np.full(n, np.inf) if anchor_d2 is None else np.asarray(anchor_d2, dtype=np.float64).copy()
    taken = np.zeros(n, bool)
    order = np.full(n_select, -1, np.int32)
    gain2 = np.zeros(n_select, np.float64)
    gap = np.full(n_select, np.inf)
    undecided = np.zeros(n_select, bool)
    count = n_select
    for t in range(n_select):
        if t == 0 and first >= 0:
            p = int(first)                                           # taken as given: no mask, no min_gain2
        else:
            cand = np.flatnonzero(elig & ~taken)
            if cand.size == 0:
                count = t
                break
            p = int(cand[np.argmax(m[cand])])                       # argmax: the first of equal maxima = the lowest row
            if m[p] < min_gain2:
                count = t
                break
            if cand.size > 1 and np.isfinite(m[p]):
                gap[t] = m[p] - m[cand[cand != p]].max()
                # dim = 1 has no summation: d2 is one correctly rounded square of a difference, the same bits in every
                # implementation, so there an exact tie is decided by the row number alike everywhere
                undecided[t] = gap[t] < 2.0 * float(bound(m[p], dim)) and not (dim == 1 and gap[t] == 0.0)
        order[t], gain2[t], taken[p] = p, m[p], True
        m = np.minimum(m, d2_to_row(x64, p))
    return order, gain2, count, m, gap, undecided


def normal(dim, n):
    """The normal family: default_rng([0, dim, n]).standard_normal cast to fp32."""
    return np.random.default_rng([0, dim, n]).standard_normal((n, dim)).astype(np.float32)


def lattice(dim, n, seed=0):
    """Integer entries in {-3 .. 3}: every difference, square and sum is exact in fp64 in any order; ties are plentiful."""
    return np.random.default_rng([1, dim, n, seed]).integers(-3, 4, size=(n, dim)).astype(np.float32)


def replay(x, order, count, eligible=None, anchor_d2=None, first=-1):
    """Independent of the yardstick's own choices: replay m along the GIVEN picks.  Returns ([(m[p], largest eligible
    not-taken value) per pick, both before the pick; for a forced first the two are m[p]], final m).  Picks must be distinct
    rows, and eligible ones unless forced."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x64.shape[0]
    elig = np.ones(n, bool) if eligible is None else np.asarray(eligible).astype(bool)
    m = np.full(n, np.inf) if anchor_d2 is None else np.asarray(anchor_d2, dtype=np.float64).copy()
    taken = np.zeros(n, bool)
    out = []
    for t in range(int(count)):
        p = int(order[t])
        assert 0 <= p < n and not taken[p], (t, p)
        if t == 0 and first >= 0:
            assert p == first
            out.append((m[p], m[p]))
        else:
            assert elig[p], (t, p)
            out.append((m[p], m[elig & ~taken].max()))
        taken[p] = True
        m = np.minimum(m, d2_to_row(x64, p))
    return out, m
