"""Per-row top-k lists out of the all-pairs pass on the MI355X (include/siggan_verifier_topk.h): every list against numpy on the
existing call's own score matrix -- integer rows and bit-equal scores, no tolerance -- for both total orders, with and without
ids and same_set, short lists, ties, every split count, chunked queries, run to run, and the refusals.

The state is verifiercommon.torch_state(e); the embeddings are those of verifier_inputs' generated images, embedded once per E
and shared (never written to)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NOISE, N_STROKE = 130, 300
KEYS = ("impostor_score", "impostor_index", "genuine_score", "genuine_index")


@functools.lru_cache(maxsize=None)
def model_of(e):
    m = SV.SiameseNetwork(e, max_images=128)
    m.load_state_dict(VC.torch_state(e), strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def pool(e):
    """(noise embeddings (130, E), stroke embeddings (300, E)) of model_of(e)."""
    m = model_of(e)
    a = m.forward_one(torch.from_numpy(VI.gen_x1(N_NOISE)).to(DEV))
    b = m.embed_u8(torch.from_numpy(VI.gen_x2_bytes(N_STROKE)).to(DEV))
    return a, b


def five_writers(n):
    """int32 ids of five writers over n rows, interleaved; writer 4 has a single signature (row 3)."""
    ids = np.arange(n) % 4
    if n > 3:
        ids[3] = 4
    return torch.from_numpy(ids.astype(np.int32)).to(DEV)


def numpy_lists(s, genuine, candidate, k, genuine_lowest):
    """The four (nq, k) arrays from the score matrix: per row the candidates of a class sorted by (score descending, column
    ascending) -- or (score ascending, column ascending) for the lowest genuine scores -- on the fp32 BITS (scores lie in
    [0, 1], where the bit pattern is monotone), the first k, padded with -1.0 / -1."""
    nq = s.shape[0]
    bits = s.view(np.int32).astype(np.int64)
    assert (bits >= 0).all()
    out = {n: (np.full((nq, k), -1.0, np.float32) if n.endswith("score") else np.full((nq, k), -1, np.int32)) for n in KEYS}
    for i in range(nq):
        for c, mask, lowest in (("impostor", ~genuine[i] & candidate[i], False), ("genuine", genuine[i] & candidate[i], genuine_lowest)):
            cols = np.flatnonzero(mask)
            order = cols[np.lexsort((cols, bits[i, cols] if lowest else -bits[i, cols]))][:k]
            out[f"{c}_score"][i, :order.size] = s[i, order]
            out[f"{c}_index"][i, :order.size] = order
    return out


def assert_lists(got, want, what):
    for n in got:
        g, w = got[n].cpu().numpy(), want[n]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, g.shape)
        assert np.array_equal(g.view(np.int32), w.view(np.int32)), f"{what}: {n}\n{g}\n{w}"


def check_against_numpy(m, q, idq, r, idr, k, same_set, genuine_lowest, what):
    """One pair_topk call against numpy on score_matrix; returns numpy's lists."""
    nq, nr = q.shape[0], r.shape[0]
    s = m.score_matrix(q, r).cpu().numpy()
    genuine = (idq.cpu().numpy()[:, None] == idr.cpu().numpy()[None, :]) if idq is not None else np.zeros((nq, nr), bool)
    candidate = ~np.eye(nq, dtype=bool) if same_set else np.ones((nq, nr), bool)
    want = numpy_lists(s, genuine, candidate, k, genuine_lowest)
    got = m.pair_topk(q, idq, r, idr, k, same_set=same_set, genuine_lowest=genuine_lowest)
    assert set(got) == set(KEYS)
    assert_lists(got, want, what)
    return want


# ------------------------------------------------------------------------------------------------------------ 1. lists == numpy
@pytest.mark.parametrize("nq,nr,e,k", [(33, 70, 128, 1), (33, 70, 128, 4), (33, 70, 128, 16), (33, 70, 40, 4), (130, 300, 128, 8),
                                       (5, 3, 7, 4)])
def test_lists_equal_numpy_on_the_matrix(nq, nr, e, k):
    m = model_of(e)
    a, b = pool(e)
    for same_set in (False, True):
        if same_set:                                                  # one ragged set against itself
            n = max(nq, nr)
            h = min(n // 2, N_NOISE)
            q = r = torch.cat([a[:h], b[:n - h]]).contiguous()
            idq = idr = five_writers(n)
        else:
            q, r, idq, idr = a[:nq].contiguous(), b[:nr].contiguous(), five_writers(nq), five_writers(nr)
        for with_ids in (True, False):
            for lowest in (True, False):
                want = check_against_numpy(m, q, idq if with_ids else None, r, idr if with_ids else None, k, same_set, lowest,
                                           f"{nq}x{nr} E={e} k={k} same_set={same_set} ids={with_ids} lowest={lowest}")
                if not with_ids:
                    assert (want["genuine_index"] == -1).all() and (want["genuine_score"] == -1.0).all()
                elif same_set and q.shape[0] > 3:
                    assert (want["genuine_index"][3] == -1).all()     # the writer with one signature has no genuine candidate
                if (nq, nr) == (5, 3):
                    if not same_set:                                  # three candidates for k = 4: padding everywhere
                        assert (want["impostor_index"][:, -1] == -1).all() and (want["impostor_score"][:, -1] == -1.0).all()
                        if with_ids:
                            assert (want["genuine_index"][3] == -1).all() and want["genuine_index"][0, 0] == 0
                    elif not with_ids:                                # four candidates for k = 4: full, no padding
                        assert (want["impostor_index"] >= 0).all()


# ------------------------------------------------------------------------------------------------------------ 2. k = 1
def test_k1_highest_is_best_matches():
    m = model_of(128)
    a, b = pool(128)
    for q, idq, r, idr, same in ((a[:41].contiguous(), five_writers(41), b[:88].contiguous(), five_writers(88), False),
                                 (b[:67].contiguous(), five_writers(67), b[:67].contiguous(), five_writers(67), True),
                                 (a[:41].contiguous(), None, b[:88].contiguous(), None, False)):
        bg, bgi, bi, bii = m.best_matches(q, idq, r, idr, same_set=same)
        out = m.pair_topk(q, idq, r, idr, 1, same_set=same, genuine_lowest=False)
        for got, want in ((out["genuine_score"], bg), (out["genuine_index"], bgi), (out["impostor_score"], bi), (out["impostor_index"], bii)):
            assert got.shape == (q.shape[0], 1) and got.dtype == want.dtype
            assert torch.equal(got[:, 0].view(torch.int32), want.view(torch.int32))
    # one class alone: the other is neither computed nor returned
    only = m.pair_topk(q, idq, r, idr, 1, want=("impostor",))
    assert set(only) == {"impostor_score", "impostor_index"} and torch.equal(only["impostor_index"][:, 0], bii)


# ------------------------------------------------------------------------------------------------------------ 3. ties
def test_ties_resolve_to_ascending_rows():
    m = model_of(128)
    a, b = pool(128)
    q = torch.cat([a[:20], b[:21]]).contiguous()
    r = torch.cat([b[:40], a[:8], b[:40]]).contiguous()               # rows 48 .. 87 repeat rows 0 .. 39
    idq = torch.from_numpy((np.arange(41) % 5).astype(np.int32)).to(DEV)
    idr = torch.from_numpy((np.arange(88) % 4).astype(np.int32)).to(DEV)
    for lowest in (True, False):
        want = check_against_numpy(m, q, idq, r, idr, 6, False, lowest, f"duplicated rows, lowest={lowest}")
        for n in ("impostor_index", "genuine_index"):
            ix = want[n]
            for i in range(41):
                for p, j in enumerate(ix[i]):
                    if 0 <= j < 40 and p + 1 < 6:                     # a duplicated row is followed by its copy, the higher row
                        assert ix[i, p + 1] == j + 48, (n, i, ix[i])
        assert (want["impostor_index"][:, 0] < 48).all()


def test_saturated_head_every_score_one():
    e, scale = 128, 1e5
    sd = VC.torch_state(e)
    sd["classifier.3.bias"] = (sd["classifier.3.bias"].abs() + 10.0) * scale
    sd["classifier.3.weight"] = sd["classifier.3.weight"].abs() * scale           # ReLU outputs are >= 0: every logit is huge
    m = SV.SiameseNetwork(e, max_images=64)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    a, b = pool(e)                                                    # the encoder's weights are model_of(e)'s
    x = torch.cat([a[:30], b[:37]]).contiguous()                      # 67 rows: three reference tiles, ragged
    assert bool((m.score_matrix(x, x) == 1.0).all()), "the case is mis-set"
    ids = five_writers(67)
    for same in (False, True):
        for lowest in (True, False):
            want = check_against_numpy(m, x, ids, x, ids, 5, same, lowest, f"saturated same_set={same} lowest={lowest}")
            for n in ("impostor_index", "genuine_index"):
                filled = want[n] >= 0
                assert (np.diff(want[n], axis=1)[filled[:, 1:]] > 0).all()        # equal scores: strictly ascending rows
            assert (want["impostor_score"] == 1.0).all()
    out = m.pair_topk(x, None, x, None, 16, same_set=True)
    ix = out["impostor_index"].cpu().numpy()
    for i in range(67):
        assert ix[i].tolist() == [j for j in range(18) if j != i][:16]           # the first 16 rows that are not the row itself


# ------------------------------------------------------------------------------------------------------------ 4. splits
def grid_splits(nq, nr):
    """siggan_verifier_pairs' split count of the reference range (csrc/verifier.hip, pair_grid)."""
    qt, ntiles = (nq + 15) // 16, (nr + 31) // 32
    return min(32, ntiles, (1024 + qt - 1) // qt) if qt < 1024 else 1


@pytest.mark.parametrize("nq,nr,splits", [(1, 2000, 32), (130, 2000, 32), (130, 70, 3), (1, 33, 2)])
def test_lists_do_not_depend_on_the_split(nq, nr, splits):
    assert grid_splits(nq, nr) == splits
    m = model_of(128)
    a, b = pool(128)
    x = torch.cat([a, b])
    g = torch.Generator().manual_seed(5)
    i1, i2 = torch.randint(0, 430, (nr,), generator=g).to(DEV), torch.randint(0, 430, (nr,), generator=g).to(DEV)
    r = (0.5 * (x[i1] + x[i2])).contiguous()                          # embedding-like rows, as many as asked for
    r[nr // 2] = r[1]                                                 # one tie across two splits
    q = a[:nq].contiguous()
    idq = torch.from_numpy((np.arange(nq) % 7).astype(np.int32)).to(DEV)
    idr = torch.from_numpy((np.arange(nr) % 7).astype(np.int32)).to(DEV)
    for k in (1, 16):
        want = check_against_numpy(m, q, idq, r, idr, k, False, True, f"{nq}x{nr} k={k}: {splits} splits")
        assert (want["impostor_index"][:, 0] >= 0).all()
    if nr == 2000:
        assert len({int(t) // 2 for t in want["impostor_index"][0] // 32}) > 1        # two tiles per split: the list spans several


# ------------------------------------------------------------------------------------------------------------ 5. / 6.
@pytest.mark.parametrize("same_set", [False, True])
def test_chunked_queries_equal_unchunked(same_set, monkeypatch):
    m = model_of(128)
    a, b = pool(128)
    if same_set:
        q = r = torch.cat([a[:25], b[:25]]).contiguous()
        idq = idr = five_writers(50)
    else:
        q, r, idq, idr = a[:50].contiguous(), b[:70].contiguous(), five_writers(50), five_writers(70)
    for k in (4, 16):
        for ids in ((idq, idr), (None, None)):
            whole = m.pair_topk(q, ids[0], r, ids[1], k, same_set=same_set)
            monkeypatch.setattr(SV, "PAIR_TOPK_CHUNK", 16)            # 16 + 16 + 16 + 2 rows
            parts = m.pair_topk(q, ids[0], r, ids[1], k, same_set=same_set)
            monkeypatch.undo()
            assert SV.PAIR_TOPK_CHUNK == 4096
            for n in KEYS:
                assert parts[n].shape == whole[n].shape and parts[n].dtype == whole[n].dtype
                assert torch.equal(parts[n].view(torch.int32), whole[n].view(torch.int32)), (n, k, same_set)


def test_run_to_run_bits():
    m = model_of(128)
    a, b = pool(128)
    q, r, idq, idr = a[:130].contiguous(), b[:300].contiguous(), five_writers(130), five_writers(300)
    o1 = m.pair_topk(q, idq, r, idr, 16)
    o2 = m.pair_topk(q, idq, r, idr, 16)
    m.score_matrix(q[:3], r[:5])                                      # an unrelated call on the same context
    o3 = m.pair_topk(q, idq, r, idr, 16)
    for n in KEYS:
        assert torch.equal(o1[n].view(torch.int32), o2[n].view(torch.int32)) and torch.equal(o1[n].view(torch.int32), o3[n].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 7. refusals
PAD_F, PAD_I = 7.25, 123456


class Outputs:
    def __init__(self, n, k):
        self.t = {n_: (torch.full((n, k), PAD_F, device=DEV) if n_.endswith("score") else torch.full((n, k), PAD_I, dtype=torch.int32, device=DEV))
                  for n_ in KEYS}

    def struct(self, names=KEYS, shift=0):
        o = _lib.PairTopk()
        for n in names:
            setattr(o, n + "_dev", self.t[n].data_ptr() + shift)
        return o

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == (PAD_F if n.endswith("score") else PAD_I)).all()) for n, t in self.t.items())


def raw_call(ctx, q, r, nq, nr, same_set, k, o):
    return ctx.lib.siggan_verifier_pairs_topk(ctx._h, C.c_void_p(q.data_ptr()), None, nq, C.c_void_p(r.data_ptr()), None, nr, same_set, k, 1,
                                              C.byref(o), ctx._stream())


def test_refusals_leave_the_outputs_untouched():
    e = 128
    a, b = pool(e)
    q, r = a[:5].contiguous(), b[:7].contiguous()
    out = Outputs(8, 4)
    lib = _lib.load()

    def refused(rc, what):
        assert rc == _lib.E_ARG, what
        assert lib.siggan_last_error(), what
        assert out.untouched(), f"'{what}' wrote to the outputs"

    weights = [p.to(DEV) for k_, p in VC.torch_state(e).items() if not k_.endswith("num_batches_tracked")]
    # before bind, before either enable
    ctx = SV._Context(DEV, e, 4)
    refused(lib.siggan_verifier_pairs_topk_enable(ctx._h, 8, 4), "topk_enable before pairs_enable")
    assert lib.siggan_verifier_pairs_enable(ctx._h, 1) == 0 and lib.siggan_verifier_pairs_topk_enable(ctx._h, 6, 4) == 0
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, out.struct()), "before bind")
    ctx.close()
    ctx = SV._Context(DEV, e, 4)
    ctx.bind(weights, VC.BN_EPS)
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, out.struct()), "before pairs_enable")
    assert lib.siggan_verifier_pairs_enable(ctx._h, 1) == 0
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, out.struct()), "before topk_enable")
    for rows, kmax, what in ((0, 4, "max_queries = 0"), (6, 0, "max_k = 0"), (6, 17, "max_k = 17")):
        refused(lib.siggan_verifier_pairs_topk_enable(ctx._h, rows, kmax), what)
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, out.struct()), "after refused enables")
    assert lib.siggan_verifier_pairs_topk_enable(ctx._h, 6, 4) == 0
    refused(raw_call(ctx, q, r, 5, 7, 0, 0, out.struct()), "k = 0")
    refused(raw_call(ctx, q, r, 5, 7, 0, 5, out.struct()), "k above max_k")
    refused(raw_call(ctx, r, q, 7, 5, 0, 4, out.struct()), "nq above max_queries")
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, _lib.PairTopk()), "no output requested")
    refused(raw_call(ctx, q, r, 5, 7, 1, 4, out.struct()), "same_set with nq != nr")
    refused(raw_call(ctx, q, r, 0, 7, 0, 4, out.struct()), "nq = 0")
    mis = torch.empty(5 * e + 1, dtype=torch.float32, device=DEV)[1:]
    refused(raw_call(ctx, mis, r, 5, 7, 0, 4, out.struct()), "misaligned embeddings")
    refused(raw_call(ctx, q, r, 5, 7, 0, 4, out.struct(shift=2)), "misaligned outputs")
    refused(ctx.lib.siggan_verifier_pairs_topk(ctx._h, None, None, 5, C.c_void_p(r.data_ptr()), None, 7, 0, 4, 1, C.byref(out.struct()), None),
            "null embeddings")
    # and then a valid call: only the requested class is written, rows beyond nq stay
    assert raw_call(ctx, q, r, 5, 7, 0, 4, out.struct(("impostor_score", "impostor_index"))) == 0
    torch.cuda.synchronize()
    want = numpy_lists(model_of(e).score_matrix(q, r).cpu().numpy(), np.zeros((5, 7), bool), np.ones((5, 7), bool), 4, True)
    assert np.array_equal(out.t["impostor_score"][:5].cpu().numpy().view(np.int32), want["impostor_score"].view(np.int32))
    assert np.array_equal(out.t["impostor_index"][:5].cpu().numpy(), want["impostor_index"])
    assert bool((out.t["impostor_index"][5:] == PAD_I).all()) and bool((out.t["genuine_index"] == PAD_I).all())
    assert bool((out.t["genuine_score"] == PAD_F).all())
    # growing max_k keeps max_queries, and the other way round
    assert lib.siggan_verifier_pairs_topk_enable(ctx._h, 1, 16) == 0
    big = Outputs(5, 16)
    assert raw_call(ctx, q, r, 5, 7, 0, 16, big.struct()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(big.t["impostor_index"].cpu().numpy()[:, :4], want["impostor_index"])
    ctx.close()

    # the module's own refusals, before anything is allocated
    m = model_of(e)
    for kw in (dict(k=0), dict(k=17), dict(k=2.0), dict(k=4, want=()), dict(k=4, want=("best",)), dict(k=4, same_set=True)):
        with pytest.raises(ValueError):
            m.pair_topk(q, None, r, None, **kw)
    with pytest.raises(ValueError):
        m.pair_topk(q, five_writers(5).long(), r, None, 4)
