"""The numpy restatement of the library's RNG (rngcommon.py) held to what is known independently of the kernels: Random123's
known answers, u01 at the edges of its range, disjoint draws of the consumers listed in SITES, the planted edge seeds -- and
that the (seed, offset, shape) cases test_rng_gpu.py runs tell every mistake it is meant to catch from the right generator.
No GPU; well under a second."""
import numpy as np
import pytest

import rngcommon as R


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in R.philox4x32_10(ctr, key)) == want
    both = R.philox4x32_10(tuple(np.array([a, b], np.uint64) for a, b in zip(kat[0][0], kat[1][0])),
                           tuple(np.array([a, b], np.uint64) for a, b in zip(kat[0][1], kat[1][1])))
    assert [tuple(int(x) for x in row) for row in both] == [kat[0][2], kat[1][2]], "vectorised call"


def test_draw_raw_layout():
    """counter = (idx lo, idx hi, sid, ctr lo), key = (seed lo, seed hi ^ ctr hi)."""
    seed, ctr, idx, sid = 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0x1122334455667788, 0x56540002
    want = R.philox4x32_10((0x55667788, 0x11223344, sid, 0x76543210), (0x89ABCDEF, 0x01234567 ^ 0xFEDCBA98))
    assert np.array_equal(R.draw_raw(seed, ctr, idx, sid), want)
    assert np.array_equal(R.draw_raw(seed, ctr, np.array([idx], np.uint64), sid)[0], want)


def test_u01_edges():
    top = [0, 1, 0x7FFFFF, 0x800000, 0x800001, 0xFFFFFE, 0xFFFFFF]
    u = R.u01(np.array([t << 8 for t in top], np.uint32))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.float32(1.0)
    assert np.all(np.diff(u) >= 0)
    assert u[2] < np.float32(0.5) and u[3] == np.float32(0.5), "x >> 8 == 0x800000 is the one value with u01 == 0.5f"
    assert u[4] > np.float32(0.5) and u[5] == np.float32(1.0) - np.float32(2.0 ** -23), "the largest u01 below 1"
    assert np.array_equal(R.u01(np.array([0xFF, 0x100], np.uint32)), np.float32([2.0 ** -25, 1.5 * 2.0 ** -24])), "low 8 bits unused"
    # below 2^23 the sum is exact: u01 is (t + 0.5) / 2^24 without rounding
    t = np.array([1, 12345, 0x7FFFFF], np.uint32)
    assert np.array_equal(R.u01(t << np.uint32(8)).astype(np.float64), (t.astype(np.float64) + 0.5) / 2.0 ** 24)


def test_keep_is_the_indexed_word():
    seed, ctr, sid = 99, 7, R.SID_FC1
    w = R.draw_raw(seed, ctr, np.arange(3, dtype=np.uint64), sid).reshape(-1)
    i = np.arange(12)
    assert np.array_equal(R.keep(seed, ctr, i, sid, R.KEEP_FC), R.u01(w) < R.KEEP_FC)
    assert np.array_equal(R.keep_range(seed, ctr, sid, 3, 7, R.KEEP_FC), (R.u01(w) < R.KEEP_FC)[3:10])
    assert bool(R.keep(seed, ctr, 5, sid, R.KEEP_FC)) == bool(R.u01(w[5]) < R.KEEP_FC)


def test_normal4_against_scalar_math():
    import math
    w = R.draw_raw(5, 6, np.arange(4, dtype=np.uint64), R.SID_Z)
    got = R.normal4(w)
    for g in range(4):
        u = [float(R.u01(w[g, j])) for j in range(4)]
        for h in (0, 1):
            r, a = math.sqrt(-2.0 * math.log(u[2 * h])), 2.0 * math.pi * u[2 * h + 1]
            assert abs(got[g, 2 * h] - r * math.cos(a)) < 1e-14 and abs(got[g, 2 * h + 1] - r * math.sin(a)) < 1e-14
    d32 = np.abs(R.normal4_f32(w).astype(np.float64) - got).max()
    assert 0 < d32 < 1e-5


# ---- distinct sites ---------------------------------------------------------------------------------------------------------
def _overlaps(draws):
    out = []
    for i, a in enumerate(draws):
        for b in draws[i + 1:]:
            if (a.sid, a.ctr) == (b.sid, b.ctr) and a.e0 < b.e0 + b.n and b.e0 < a.e0 + a.n:
                out.append((a, b))
    return out


@pytest.mark.parametrize("batch", R.NOISE_BATCHES + R.LATENT_BATCHES)
def test_sites_do_not_overlap_within_a_step(batch):
    ids = [R.SID_Z, R.SID_ZG, R.SID_RANDN, R.SID_FC1, R.SID_FC2, R.SID_CLS] + [R.SID_DROP0 + l for l in range(1, 9)]
    assert len(set(ids)) == len(ids), "two consumers share a stream id"
    for c in (0, 5, (1 << 32) - 1):
        draws = R.engine_step_draws(c, batch, R.NOISE_LATENT, R.D_CHANS, staged=True) + R.randn_draws(c, 4099)
        assert not _overlaps(draws)
        z, zg = draws[0], draws[1]
        assert z.sid != zg.sid and (z.ctr, z.e0, z.n) == (zg.ctr, zg.e0, zg.n), "z and z_g: two streams, same elements"
        for l, ch in enumerate(R.D_CHANS, 1):
            p0, p1 = [d for d in draws if d.sid == R.SID_DROP0 + l and d.ctr == c]
            assert p0.e0 + p0.n == p1.e0, "the two D passes are adjacent, disjoint element ranges of one stream"
            assert p0.e0 % 4 == 0 and p1.e0 % 4 == 0, "a pass starts on a group boundary (k_dropnoise_multi)"
    for n in R.TRAINER_PAIRS:
        assert not _overlaps(R.trainer_step_draws(5, 0, n) + R.trainer_step_draws(5, 1, n))


def test_overlap_check_sees_a_shared_stream():
    draws = R.engine_step_draws(3, 4, 100, R.D_CHANS)
    shared = [d._replace(sid=R.SID_Z) if d.site == "engine.z_g" else d for d in draws]
    assert len(_overlaps(shared)) == 1
    one_pass = [d._replace(e0=0) for d in draws]
    assert len(_overlaps(one_pass)) == len(R.D_CHANS)


# ---- the GPU tests' cases tell the mutants apart ------------------------------------------------------------------------------
def _steps():
    for seed, offset, steps in R.SEEDS:
        for k in range(steps):
            yield seed, offset + k


def _mutants(seed, ctr):
    """name -> (kwargs of the restatement, counter): every mistake a case must expose."""
    m = {"nine rounds": (dict(rounds=9), ctr), "neighbouring stream id": (dict(sid_add=1), ctr), "counter + 1": ({}, ctr + 1),
         "group + 1": (dict(group_add=1), ctr)}
    if seed >> 32 or ctr >> 32:
        m["key high half ignored"] = (dict(key_high=False), ctr)
    return m


def _frac(a, b):
    return float(np.mean(np.asarray(a) != np.asarray(b)))


@pytest.mark.parametrize("n_pairs", R.TRAINER_PAIRS)
def test_trainer_mask_cases_expose_every_mutant(n_pairs):
    high = 0
    for seed, ctr in _steps():
        fc, cls = R.trainer_masks(seed, ctr, n_pairs)
        assert set(np.unique(fc)) <= {0, 1} and fc.shape == (2 * n_pairs, 512) and cls.shape == (n_pairs, 64)
        for name, (kw, c) in _mutants(seed, ctr).items():
            mfc, mcls = R.trainer_masks(seed, c, n_pairs, **kw)
            assert _frac(fc, mfc) >= 0.01 and _frac(cls, mcls) >= 0.01, (name, seed, ctr)
            high += name == "key high half ignored"
        assert _frac(fc[:n_pairs], fc[n_pairs:]) >= 0.01, "x1 and x2 share a mask"
    assert high == 2, "the seed with a high half and the step at counter 2^32 are the two key-high cases"


@pytest.mark.parametrize("batch", R.NOISE_BATCHES)
def test_dropout_table_cases_expose_every_mutant(batch):
    for seed, ctr in (list(_steps()) if batch == R.NOISE_BATCHES[0] else [(R.SEEDS[0][0], R.SEEDS[0][1])]):
        for l, ch in enumerate(R.D_CHANS, 1):
            t = R.d_noise(seed, ctr, l, batch, ch)
            assert t.shape == (2 * batch, ch) and set(np.unique(t)) <= {np.float32(0), np.float32(1) / np.float32(0.75)}
            for name, (kw, c) in _mutants(seed, ctr).items():
                assert _frac(t, R.d_noise(seed, c, l, batch, ch, **kw)) >= 0.01, (name, seed, ctr, l)
            assert _frac(t[:batch], t[batch:]) >= 0.01, "D(real) and D(fake) share a table"
            # pass 1 is the continuation of pass 0's stream, not a second copy from element 0
            assert np.array_equal(t[batch:], R.d_noise(seed, ctr, l, batch, ch, passes=(1,)))


def test_latent_cases_expose_every_mutant():
    """Raw words: every group differs under every mutant (and z from z_g)."""
    cases = [(R.LATENT_SEED[0], R.LATENT_SEED[1], sid, b * R.NOISE_LATENT) for b in R.LATENT_BATCHES + (R.LATENT_FALLBACK,)
             for sid in (R.SID_Z, R.SID_ZG)]
    cases += [(R.RANDN_SEED[0], R.RANDN_SEED[1] + 1, R.SID_RANDN, n) for n in R.RANDN_N]
    for seed, ctr, sid, n in cases:
        g = np.arange((n + 3) // 4, dtype=np.uint64)
        w = R.draw_raw(seed, ctr, g, sid)
        for name, m in (("nine rounds", R.draw_raw(seed, ctr, g, sid, rounds=9)), ("neighbouring stream id", R.draw_raw(seed, ctr, g, sid + 1)),
                        ("counter + 1", R.draw_raw(seed, ctr + 1, g, sid)), ("group + 1", R.draw_raw(seed, ctr, g + np.uint64(1), sid))):
            assert np.all(np.any(w != m, axis=-1)), (name, sid, n)
        # ... and the difference is far outside the parity bound in the normals themselves
        z = R.normals(seed, ctr, sid, n)
        assert np.abs(z - R.normals(seed, ctr, sid, n, group_add=1)).max() > 1e-3


def test_le_mutant_needs_the_planted_tie():
    """`<=` for `<` differs only where u01 == keep exactly.  None of the regular cases has such an element; the planted
    trainer seed has exactly one, and the GPU test runs it."""
    for seed, ctr in _steps():
        for n in R.TRAINER_PAIRS:
            a, b = R.trainer_masks(seed, ctr, n), R.trainer_masks(seed, ctr, n, strict=False)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    e = R.EDGE_KEEP_TIE
    sid = (R.SID_FC1, R.SID_FC2)[e["site"]]
    w = R.draw_raw(e["seed"], e["offset"], e["element"] >> 2, sid)[e["element"] & 3]
    assert int(w) >> 8 == 0x800000 and R.u01(w) == R.KEEP_FC
    assert not R.keep(e["seed"], e["offset"], e["element"], sid, R.KEEP_FC)
    assert R.keep(e["seed"], e["offset"], e["element"], sid, R.KEEP_FC, strict=False)
    fc, _ = R.trainer_masks(e["seed"], e["offset"], e["n_pairs"])
    fc_le, _ = R.trainer_masks(e["seed"], e["offset"], e["n_pairs"], strict=False)
    row, col = e["site"] * e["n_pairs"] + e["element"] // 512, e["element"] % 512
    diff = np.argwhere(fc != fc_le)
    assert diff.tolist() == [[row, col]] and fc[row, col] == 0 and fc_le[row, col] == 1


def test_planted_radius_edges():
    for e, top, u in ((R.EDGE_U_ONE, 0xFFFFFF, 1.0), (R.EDGE_U_MIN, 0, 2.0 ** -25), (R.EDGE_U_TOP, 0xFFFFFE, 1.0 - 2.0 ** -23)):
        el = e["element"]
        assert el % 2 == 0 and el + 1 < R.EDGE_N, "the first normal of a half-group inside the first 4096 elements"
        w = R.draw_raw(e["seed"], e["offset"] + 1, el >> 2, R.SID_RANDN)              # op_randn ticks, then draws
        assert int(w[el & 3]) >> 8 in (top, top - (top == 0xFFFFFE)) and R.u01(w[el & 3]) == np.float32(u)
        z = R.normals(e["seed"], e["offset"] + 1, R.SID_RANDN, R.EDGE_N)
        assert np.all(np.isfinite(z))
        r = np.hypot(z[el], z[el + 1])
        if top == 0xFFFFFF:
            assert z[el] == 0.0 and z[el + 1] == 0.0
            z32 = R.normals(e["seed"], e["offset"] + 1, R.SID_RANDN, R.EDGE_N, f32=True)
            assert z32[el] == 0.0 and z32[el + 1] == 0.0 and np.all(np.isfinite(z32))
        elif top == 0xFFFFFE:
            assert abs(r - np.sqrt(-2.0 * np.log1p(-2.0 ** -23))) < 1e-15 and 0.99 * 2.0 ** -11 < r < 1.01 * 2.0 ** -11
        else:
            assert abs(r - np.sqrt(50.0 * np.log(2.0))) < 1e-12 and abs(r - 5.887) < 1e-3
            assert np.abs(z).max() <= r + 1e-12, "2^-25 is the smallest u: no larger radius exists"
