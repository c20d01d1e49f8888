"""The yardstick of k-means (include/siggan_kmeans.h): the header restated in numpy fp64 -- the two-level sum, the uniform
of a seeding step, the D^2 sampling rule with its two fallbacks, one Lloyd pass with direct fp64 distances and the sequential
centre sum --, the error bounds, and the input families the CPU and GPU tests share.

Bounds (derived, not tuned).  Assignment: the device forms d2 = (|x|^2 + |c|^2) - 2 x.c, the yardstick sums squared
differences; tests/test_neighbors_gpu.py's B_ij = (dim + 4) * 2^-52 * (|x_i| + |c_j|)^2 bounds their distance.  Seeding: both
sides sum squared differences, diversecommon.bound (B = (dim + 4) * 2^-52 * d2) bounds the distance of two evaluations of one
m[i]; a prefix of i + 1 such values, summed in any order, adds (i + 1) roundings of at most 2^-53 of the prefix on either
side, so two evaluations of prefix_i differ by at most E_i = sum_{j <= i} B(m_j) + (i + 2) * 2^-52 * prefix_i, and of the
target u * T by at most u * E_(n-1) + 2^-52 * target.

A comparison is "undecided" when it is decided by less than twice its bound: another correct implementation may then decide
it the other way, and the tests that compare decisions exactly must pick another seed."""
import numpy as np

import diversecommon as D
import rngcommon as R
from diversecommon import lattice, normal  # noqa: F401  (the families the tests share)

SID_KMEANS = 0x4B4D5050                                      # "KMPP"
SUM_BLOCK = 64
EPS = 2.0 ** -52


def two_level(v):
    """(total, prefix (n,)) of the header's two-level sum of v (n,) fp64.  np.cumsum is a sequential loop in ascending order;
    0.0 + v[0] == v[0], and the zeros that pad the last block add exactly nothing."""
    v = np.asarray(v, dtype=np.float64)
    n = v.size
    blocks = -(-n // SUM_BLOCK)
    padded = np.zeros(blocks * SUM_BLOCK)
    padded[:n] = v
    running = np.cumsum(padded.reshape(blocks, SUM_BLOCK), axis=1)            # r_i inside every block
    q = np.cumsum(running[:, -1])                                             # Q_b
    before = np.concatenate([[0.0], q[:-1]])                                  # Q_(b-1)
    prefix = (before[:, None] + running).reshape(-1)[:n]
    return float(q[-1]), prefix


def two_level_slow(v):
    """The same sum in plain Python floats, line for line as the header states it (test_kmeans_cpu holds two_level to it)."""
    v = [float(a) for a in v]
    q, prefix = 0.0, []
    for b in range(0, len(v), SUM_BLOCK):
        r = 0.0
        for a in v[b:b + SUM_BLOCK]:
            r = r + a
            prefix.append(q + r)
        q = q + r
    return q, np.array(prefix)


def uniform(seed, s):
    """u_s = ((w.x >> 5) * 2^26 + (w.y >> 6)) * 2^-53 of the word draw_raw(seed, ctr = s, idx = 0, SID_KMEANS): every step
    exact in fp64."""
    w = R.draw_raw(seed, s, 0, SID_KMEANS).reshape(-1)
    return (float(int(w[0]) >> 5) * 67108864.0 + float(int(w[1]) >> 6)) * 2.0 ** -53


def seed_rows(x, k, seed):
    """(rows int32 (k,), steps): the seeding rule.  steps[s] (s >= 1) = dict(total, target, rule in {'prefix', 'last',
    'unchosen'}, margin, bound): margin = how far the target is from the nearer of the two prefixes around the crossing,
    bound = the accumulated bound of that comparison (both 0 for the rules that compare nothing inexact)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, dim = x64.shape
    rows = np.zeros(k, np.int32)
    rows[0] = min(n - 1, int(np.floor(uniform(seed, 0) * n)))
    m = np.full(n, np.inf)
    steps = [None]
    for s in range(1, k):
        m = np.minimum(m, D.d2_to_row(x64, rows[s - 1]))
        total, prefix = two_level(m)
        u = uniform(seed, s)
        target = u * total
        info = dict(total=total, target=target, margin=np.inf, bound=0.0)
        if total == 0.0:
            chosen = set(rows[:s].tolist())
            row, info["rule"] = next(r for r in range(n) if r not in chosen), "unchosen"
        else:
            err = np.cumsum(D.bound(m, dim)) + (np.arange(n) + 2) * EPS * prefix
            target_err = u * err[-1] + EPS * target
            over = np.flatnonzero(prefix > target)
            if over.size:
                row, info["rule"] = int(over[0]), "prefix"
                info["margin"], info["bound"] = prefix[row] - target, err[row] + target_err
                if row > 0 and target - prefix[row - 1] < info["margin"]:
                    info["margin"], info["bound"] = target - prefix[row - 1], err[row - 1] + target_err
            else:
                row, info["rule"] = int(np.flatnonzero(m > 0)[-1]), "last"
                info["margin"], info["bound"] = 0.0, err[-1] + target_err     # decided by rounding alone: always undecided
        rows[s] = row
        steps.append(info)
    return rows, steps


def seeding_is_decided(steps):
    return all(st is None or st["rule"] == "unchosen" or st["margin"] >= 2.0 * st["bound"] for st in steps)


def assign_bound(x64, c64):
    """B_ij (n, k)."""
    dim = x64.shape[1]
    xn, cn = np.sqrt((x64 ** 2).sum(1)), np.sqrt((c64 ** 2).sum(1))
    return (dim + 4) * EPS * (xn[:, None] + cn[None, :]) ** 2


def distances(x64, c64):
    """(n, k) direct fp64 squared distances, one centre at a time (the (n, k, dim) block is never formed)."""
    return np.stack([((x64 - c) ** 2).sum(1) for c in c64], axis=1)


def assign(x, centres):
    """(labels int32 (n,), mind2 (n,), undecided bool (n,), bound (n,)): the nearest centre by direct fp64 distances, equal
    ones to the lower centre; undecided: the runner-up is closer than twice the larger of the two bounds."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(centres, dtype=np.float32).astype(np.float64)
    d2, b = distances(x64, c64), assign_bound(x64, c64)
    labels = np.argmin(d2, axis=1).astype(np.int32)                           # argmin: the first of equal minima
    rows = np.arange(len(x64))
    mind2, own = d2[rows, labels], b[rows, labels]
    undecided = np.zeros(len(x64), bool)
    if c64.shape[0] > 1 and not exact(x64, c64):
        rest = d2.copy()
        rest[rows, labels] = np.inf
        second = np.argmin(rest, axis=1)
        undecided = rest[rows, second] - mind2 < 2.0 * np.maximum(own, b[rows, second])
    return labels, mind2, undecided, own


def exact(x64, c64):
    """Every value an integer of small size: all of the device's and the yardstick's arithmetic is exact, ties are real ties
    and go to the lower centre on both sides."""
    return bool(np.all(x64 == np.round(x64)) and np.all(c64 == np.round(c64)) and np.abs(x64).max(initial=0) <= 1024
                and np.abs(c64).max(initial=0) <= 1024)


def update(x, labels, centres):
    """The centre update: per centre the fp64 sum of its rows in ascending row number (np.cumsum along the rows is that
    sequential sum), divided by the count, rounded to fp32; a centre without rows keeps its bits.  -> (centres fp32, counts)."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    out = np.array(centres, dtype=np.float32, copy=True)
    counts = np.bincount(labels, minlength=len(out)).astype(np.int32)
    for j in np.flatnonzero(counts):
        total = np.cumsum(x64[labels == j], axis=0)[-1]
        out[j] = (total / float(counts[j])).astype(np.float32)
    return out, counts


def inertia(mind2):
    return two_level(mind2)[0]


def inertia_bound(bounds, mind2):
    """Two evaluations of the two-level sum of n values that differ by at most bounds[i] each."""
    n = len(mind2)
    return float(np.sum(bounds) + (n + 2) * EPS * np.sum(mind2))


def blob_centres(dim, k, seed=0, spread=12.0):
    """spread * standard normal: about spread * sqrt(2 dim) apart against a blob radius of sqrt(dim)."""
    return spread * np.random.default_rng([2, dim, k, seed]).standard_normal((k, dim))


def blobs(dim, n, k, seed=0, draw=0, weights=None):
    """(x fp32 (n, dim), blob (n,)): k well-separated unit-variance normal clusters of unequal size around blob_centres(dim, k,
    seed).  Blob j's share is weights[j] (default j + 1, normalised; 0 leaves the blob out); ``draw`` names the sample, so two
    draws share the centres and nothing else.  Rows come in a seeded random order."""
    rng = np.random.default_rng([3, dim, n, k, seed, draw])
    w = np.arange(1, k + 1, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    edges = np.floor(np.cumsum(w / w.sum()) * n + 0.5).astype(np.int64)
    edges[-1] = n
    blob = np.searchsorted(edges, np.arange(n), side="right").astype(np.int64)
    x = blob_centres(dim, k, seed)[blob] + rng.standard_normal((n, dim))
    order = rng.permutation(n)
    return x[order].astype(np.float32), blob[order]
