"""All-pairs scoring on the MI355X (include/siggan_verifier_pairs.h): the score matrix bit for bit against siggan_verifier_compare
on the expanded pair list and within verifiercommon's bound of the fp64 head; the threshold histograms and the row maxima against
numpy on the call's own matrix; saturation, determinism, one pass for all outputs, the refusals, and evaluate_all_pairs / the CLI
against compute_verification_metrics on the scores of every pair.

The state is verifiercommon.torch_state(e); the embeddings are those of verifier_inputs' generated images (uniform-noise fp32
images first, stroke-like byte images after them), embedded once per E and shared."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import verifiercommon as VC
from verifiercommon import VI

import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd import signature_verifier_eval as SV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NOISE, N_STROKE = 130, 300
FIXTURE_OF = {128: (33, 128), 40: (3, 40)}          # the fixture whose similarity bound stands for an embedding width


def i32(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def model_of(e):
    m = SV.SiameseNetwork(e, max_images=128)
    m.load_state_dict(VC.torch_state(e), strict=True)
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def pool(e):
    """(noise embeddings (130, E), stroke embeddings (300, E)) of model_of(e); never written to."""
    m = model_of(e)
    a = m.forward_one(torch.from_numpy(VI.gen_x1(N_NOISE)).to(DEV))
    b = m.embed_u8(torch.from_numpy(VI.gen_x2_bytes(N_STROKE)).to(DEV))
    return a, b


def expanded_compare(m, q, r):
    nq, nr = q.shape[0], r.shape[0]
    qi = torch.arange(nq, device=DEV).repeat_interleave(nr)
    rj = torch.arange(nr, device=DEV).repeat(nq)
    return m.compare(q[qi], r[rj]).view(nq, nr), qi, rj


def five_writers(n):
    """int32 ids of five writers over n rows, interleaved; writer 4 has a single signature (row 3)."""
    ids = np.arange(n) % 4
    ids[3] = 4
    return torch.from_numpy(ids.astype(np.int32)).to(DEV)


def numpy_counts(s, genuine, thr):
    b = np.searchsorted(thr, s, side="right")
    n = thr.size + 1
    return np.bincount(b[genuine], minlength=n), np.bincount(b[~genuine], minlength=n)


def numpy_best(s, genuine, candidate):
    """Per row: (best genuine, its column, best impostor, its column); the first of equal maxima; (-1, -1) without a candidate."""
    nq = s.shape[0]
    out = [np.full(nq, -1.0, np.float32), np.full(nq, -1, np.int32), np.full(nq, -1.0, np.float32), np.full(nq, -1, np.int32)]
    for i in range(nq):
        for c, mask in enumerate((genuine[i] & candidate[i], ~genuine[i] & candidate[i])):
            if mask.any():
                j = int(np.argmax(np.where(mask, s[i], -np.inf)))
                out[2 * c][i], out[2 * c + 1][i] = s[i, j], j
    return out


BEST_KEYS = ("best_genuine", "best_genuine_index", "best_impostor", "best_impostor_index")


def assert_best(out, want, what):
    for k, w in zip(BEST_KEYS, want):
        got = out[k].cpu().numpy()
        assert got.dtype == w.dtype and np.array_equal(got.view(np.int32), w.view(np.int32)), f"{what}: {k}\n{got}\n{w}"


# ------------------------------------------------------------------------------------------------------------ 1. the matrix
@pytest.mark.parametrize("nq,nr,e", [(33, 70, 128), (33, 70, 40), (5, 3, 7), (130, 300, 128)])
def test_matrix_is_compare_bit_for_bit(nq, nr, e):
    m = model_of(e)
    a, b = pool(e)
    q, r = a[:nq].contiguous(), b[:nr].contiguous()
    s = m.score_matrix(q, r)
    assert s.shape == (nq, nr) and s.dtype == torch.float32
    want, qi, rj = expanded_compare(m, q, r)
    diff = int((i32(s) != i32(want)).sum())
    sd64 = VC.torch_state(e, dtype=torch.float64)
    ref = VC.head(sd64, q.cpu().double()[qi.cpu()], r.cpu().double()[rj.cpu()]).view(nq, nr)
    dev = float((s.cpu().double() - ref).abs().max())
    bound = VC.bound(VC.load_case(*FIXTURE_OF[e]), "similarity") if e in FIXTURE_OF else VC.CAP
    print(f"pairs {nq}x{nr} E={e}: {diff} of {nq * nr} elements differ from compare; fp64 deviation {dev:.3e} bound {bound:.3e}; "
          f"scores in [{float(s.min()):.4f}, {float(s.max()):.4f}]")
    assert torch.equal(i32(s), i32(want)), f"{diff} of {nq * nr} elements differ from siggan_verifier_compare"
    assert dev <= bound, f"fp64 deviation {dev:.3e} exceeds {bound:.3e}"


# ------------------------------------------------------------------------------------------------------------ 2. the counts
def threshold_lists(s):
    """Several of the actual scores (ties fall on an edge) plus 0.0 and 1.0; one threshold; 4096 of them."""
    d = np.unique(s)
    some = np.unique(np.concatenate([d[:: max(1, d.size // 9)], [0.0, 1.0]]).astype(np.float32))
    lattice = np.setdiff1d(np.linspace(0.0, 1.0, 6000).astype(np.float32), d[:64])
    wide = np.unique(np.concatenate([lattice[np.linspace(0, lattice.size - 1, 4096 - d[:64].size).astype(int)], d[:64]]))
    return {"scores": some, "one": d[d.size // 2: d.size // 2 + 1], "4096": wide}


@pytest.mark.parametrize("with_ids", [True, False])
@pytest.mark.parametrize("same_set", [True, False])
def test_counts_equal_numpy_on_the_matrix(same_set, with_ids):
    e = 128
    m = model_of(e)
    a, b = pool(e)
    if same_set:
        q = r = torch.cat([a[:30], b[:37]]).contiguous()             # 67 rows: ragged, five query tiles
        idq = idr = five_writers(67)
    else:
        q, r = a[:33].contiguous(), b[:70].contiguous()
        idq, idr = five_writers(33), five_writers(70)
    nq, nr = q.shape[0], r.shape[0]
    if not with_ids:
        idq = idr = None
    first = m.pairs(q, idq, r, idr, same_set=same_set, want_matrix=True, thresholds=[0.5])
    lists = threshold_lists(first["score"].cpu().numpy())
    assert lists["one"].size == 1 and lists["4096"].size == 4096 and np.all(np.diff(lists["4096"]) > 0)
    for name, thr in lists.items():
        out = m.pairs(q, idq, r, idr, same_set=same_set, want_matrix=True, thresholds=thr)
        s = out["score"].cpu().numpy()
        assert np.array_equal(s.view(np.int32), first["score"].cpu().numpy().view(np.int32))          # always the full matrix
        genuine = (idq.cpu().numpy()[:, None] == idr.cpu().numpy()[None, :]) if with_ids else np.zeros((nq, nr), bool)
        if same_set:
            iu = np.triu_indices(nq, 1)
            sv, gv, total = s[iu], genuine[iu], nq * (nq - 1) // 2
        else:
            sv, gv, total = s.reshape(-1), genuine.reshape(-1), nq * nr
        wg, wi = numpy_counts(sv, gv, thr)
        g, im = out["genuine_counts"].cpu().numpy(), out["impostor_counts"].cpu().numpy()
        assert g.dtype == np.int64 and g.shape == (thr.size + 1,) and im.shape == (thr.size + 1,)
        assert np.array_equal(g, wg) and np.array_equal(im, wi), f"{name}: counts differ\n{g}\n{wg}\n{im}\n{wi}"
        assert int(g.sum() + im.sum()) == total
        if not with_ids:
            assert int(g.sum()) == 0
        # counts alone (with same_set the tiles below the diagonal are skipped): the same bins
        g2, i2 = (m.pair_counts(q, idq, thr) if same_set else m.pair_counts(q, idq, thr, other=r, other_ids=idr))
        assert torch.equal(g2, out["genuine_counts"]) and torch.equal(i2, out["impostor_counts"]), name
    if with_ids:
        assert int(g.sum()) > 0 and int(im.sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 3. the row maxima
def test_row_maxima_equal_numpy_on_the_matrix():
    e = 128
    m = model_of(e)
    a, b = pool(e)
    q = torch.cat([a[:20], b[:21]]).contiguous()                      # 41 queries
    r = torch.cat([b[:40], a[:8], b[:40]]).contiguous()               # 88 references; rows 48 .. 87 repeat rows 0 .. 39
    idq = torch.from_numpy((np.arange(41) % 5).astype(np.int32)).to(DEV)           # writer 4 is not among the references
    idr = torch.from_numpy((np.arange(88) % 4).astype(np.int32)).to(DEV)
    out = m.pairs(q, idq, r, idr, want_matrix=True, want_best=True)
    s = out["score"].cpu().numpy()
    genuine = idq.cpu().numpy()[:, None] == idr.cpu().numpy()[None, :]
    want = numpy_best(s, genuine, np.ones_like(genuine))
    assert_best(out, want, "q x r")
    assert (want[1][idq.cpu().numpy() == 4] == -1).all() and (want[0][idq.cpu().numpy() == 4] == -1.0).all()
    assert (want[1][idq.cpu().numpy() != 4] < 48).all() and (want[3] < 48).all()          # ties took the lower row
    dup = s[:, :40] == s[:, 48:]
    assert dup.all()                                                                     # the duplicated rows do tie
    assert_best(dict(zip(BEST_KEYS, m.best_matches(q, idq, r, idr))), want, "best_matches")

    # one set against itself: j == i is a candidate without same_set and none with it
    n = 67
    x = torch.cat([a[:30], b[:37]]).contiguous()
    ids = five_writers(n)
    genuine = ids.cpu().numpy()[:, None] == ids.cpu().numpy()[None, :]
    for same in (False, True):
        out = m.pairs(x, ids, x, ids, same_set=same, want_matrix=True, want_best=True)
        s = out["score"].cpu().numpy()
        want = numpy_best(s, genuine, ~np.eye(n, dtype=bool) if same else np.ones((n, n), bool))
        assert_best(out, want, f"same_set={same}")
        if same:
            assert want[1][3] == -1 and want[0][3] == -1.0          # the writer with one signature has no genuine candidate
        else:
            assert want[1][3] == 3
    # unlabelled: every candidate is an impostor
    out = m.pairs(q, None, r, None, want_matrix=True, want_best=True)
    assert_best(out, numpy_best(out["score"].cpu().numpy(), np.zeros((41, 88), bool), np.ones((41, 88), bool)), "no ids")
    assert bool((out["best_genuine_index"] == -1).all())


# ------------------------------------------------------------------------------------------------------------ 4. saturation
def test_saturated_head():
    e, scale, shift = 128, 1e5, 0.75
    sd = VC.torch_state(e)
    sd["classifier.3.bias"] = (sd["classifier.3.bias"] - shift) * scale
    sd["classifier.3.weight"] = sd["classifier.3.weight"] * scale
    m = SV.SiameseNetwork(e, max_images=64)
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).eval()
    a, b = pool(e)                                                    # the encoder's weights are model_of(e)'s
    x = torch.cat([a[:12], b[:12]]).contiguous()
    sd64 = {k: v.double() for k, v in sd.items()}
    xi, xj = np.divmod(np.arange(24 * 24), 24)
    d = (x.cpu().double()[xi] - x.cpu().double()[xj]).abs()
    h = torch.relu(d @ sd64["classifier.0.weight"].T + sd64["classifier.0.bias"])
    logit = (h @ sd64["classifier.3.weight"].T + sd64["classifier.3.bias"]).view(24, 24).numpy()
    assert np.abs(logit).min() > 40, "the case is mis-set"
    thr = np.array([0.0, 0.5, 1.0], np.float32)
    out = m.pairs(x, None, x, None, want_matrix=True, thresholds=thr)
    s = out["score"]
    want, _, _ = expanded_compare(m, x, x)
    assert torch.equal(i32(s), i32(want))
    sn = s.cpu().numpy()
    assert np.array_equal(sn, (logit > 0).astype(np.float32)) and (sn == 0).any() and (sn == 1).any()
    im = out["impostor_counts"].cpu().numpy()
    assert im.tolist() == [0, int((sn == 0).sum()), 0, int((sn == 1).sum())]          # [0, .5) and [1, inf): first and last of the grid
    assert int(out["genuine_counts"].sum()) == 0


# ------------------------------------------------------------------------------------------------------------ 5. / 6.
def all_outputs(m, q, idq, r, idr, thr, same_set=False):
    return m.pairs(q, idq, r, idr, same_set=same_set, want_matrix=True, thresholds=thr, want_best=True)


def assert_same(o1, o2, keys=None):
    for k in (keys or o1):
        t1, t2 = o1[k], o2[k]
        assert torch.equal(t1.view(torch.int32) if t1.dtype == torch.float32 else t1, t2.view(torch.int32) if t2.dtype == torch.float32 else t2), k


def test_determinism():
    e = 128
    m = model_of(e)
    a, b = pool(e)
    q, r = a[:130].contiguous(), b[:300].contiguous()
    idq, idr = five_writers(130), five_writers(300)
    thr = SV.default_threshold_grid(0.5)
    o1 = all_outputs(m, q, idq, r, idr, thr)
    o2 = all_outputs(m, q, idq, r, idr, thr)
    m.forward_one(torch.from_numpy(VI.gen_x1(3)).to(DEV))             # an unrelated call on the same context
    o3 = all_outputs(m, q, idq, r, idr, thr)
    assert set(o1) == {"score", "thresholds", "genuine_counts", "impostor_counts", *BEST_KEYS}
    assert_same(o1, o2)
    assert_same(o1, o3)
    assert int(o1["genuine_counts"].sum() + o1["impostor_counts"].sum()) == 130 * 300


@pytest.mark.parametrize("same_set", [False, True])
def test_one_pass_serves_all_outputs(same_set):
    e = 40
    m = model_of(e)
    a, b = pool(e)
    if same_set:
        q = r = torch.cat([a[:30], b[:37]]).contiguous()
        idq = idr = five_writers(67)
    else:
        q, r, idq, idr = a[:33].contiguous(), b[:70].contiguous(), five_writers(33), five_writers(70)
    thr = SV.default_threshold_grid(0.5)
    both = all_outputs(m, q, idq, r, idr, thr, same_set)
    assert_same(m.pairs(q, idq, r, idr, same_set=same_set, want_matrix=True), both, ["score"])
    assert_same(m.pairs(q, idq, r, idr, same_set=same_set, thresholds=thr), both, ["genuine_counts", "impostor_counts"])
    assert_same(m.pairs(q, idq, r, idr, same_set=same_set, want_best=True), both, BEST_KEYS)


# ------------------------------------------------------------------------------------------------------------ 7. refusals
def raw_call(ctx, q, r, nq, nr, same_set, **fields):
    o = _lib.PairOutputs()
    keep = []
    for k, v in fields.items():
        if isinstance(v, torch.Tensor):
            keep.append(v)
            v = v.data_ptr()
        setattr(o, k, v)
    return ctx.lib.siggan_verifier_pairs(ctx._h, C.c_void_p(q.data_ptr()), None, nq, C.c_void_p(r.data_ptr()), None, nr, same_set,
                                         C.byref(o), ctx._stream())


def test_refusals():
    e = 128
    m = model_of(e)
    a, b = pool(e)
    q, r = a[:5].contiguous(), b[:7].contiguous()
    good = m.score_matrix(q, r)
    ctx = m._context()
    s = torch.empty(5, 7, dtype=torch.float32, device=DEV)
    thr = torch.linspace(0, 1, 4097, device=DEV)
    cnt = torch.zeros(2, 4098, dtype=torch.int64, device=DEV)
    counts = dict(threshold_dev=thr, genuine_count_dev=cnt[0], impostor_count_dev=cnt[1])

    def refused(rc, what):
        assert rc == _lib.E_ARG, what
        assert ctx.lib.siggan_last_error()
        assert raw_call(ctx, q, r, 5, 7, 0, score_dev=s) == 0 and torch.equal(i32(s), i32(good)), f"after '{what}' a valid call fails"

    refused(raw_call(ctx, q, r, 5, 7, 0), "no output requested")
    refused(raw_call(ctx, q, r, 5, 7, 0, n_thresholds=0, **counts), "T = 0")
    refused(raw_call(ctx, q, r, 5, 7, 0, n_thresholds=4097, **counts), "T = 4097")
    refused(raw_call(ctx, q, r, 5, 7, 0, n_thresholds=8, threshold_dev=thr), "counts without their arrays")
    refused(raw_call(ctx, q, r, 5, 7, 1, score_dev=s), "same_set with nq != nr")
    refused(raw_call(ctx, q, r, 0, 7, 0, score_dev=s), "nq = 0")
    mis = torch.empty(5 * e + 1, dtype=torch.float32, device=DEV)[1:]
    refused(raw_call(ctx, mis, r, 5, 7, 0, score_dev=s), "misaligned embeddings")
    assert raw_call(ctx, q, r, 5, 7, 0, n_thresholds=4096, **counts) == 0 and int(cnt[:, :4097].sum()) == 35
    # the module's own refusals, before anything is allocated
    for kw in (dict(), dict(thresholds=[]), dict(thresholds=np.zeros(4097)), dict(thresholds=[0.5, 0.25]), dict(want_matrix=True, same_set=True)):
        with pytest.raises(ValueError):
            m.pairs(q, None, r, None, **kw)
    assert torch.equal(i32(m.score_matrix(q, r)), i32(good))

    # before bind
    fresh = SV._Context(DEV, e, 4)
    assert fresh.lib.siggan_verifier_pairs_enable(fresh._h, 8) == 0
    assert raw_call(fresh, q, r, 5, 7, 0, score_dev=s) == _lib.E_ARG
    with pytest.raises(ValueError, match="bind"):
        fresh.pairs(q, None, r, None, want_matrix=True)
    fresh.close()
    # before enable; row maxima beyond max_queries
    sd = VC.torch_state(e)
    weights = [p.to(DEV) for k, p in sd.items() if not k.endswith("num_batches_tracked")]
    fresh = SV._Context(DEV, e, 4)
    fresh.bind(weights, VC.BN_EPS)
    assert raw_call(fresh, q, r, 5, 7, 0, score_dev=s) == _lib.E_ARG
    assert fresh.lib.siggan_verifier_pairs_enable(fresh._h, 0) == _lib.E_ARG
    assert fresh.lib.siggan_verifier_pairs_enable(fresh._h, 4) == 0
    bi = torch.empty(5, dtype=torch.float32, device=DEV)
    assert raw_call(fresh, q, r, 5, 7, 0, best_impostor_dev=bi) == _lib.E_ARG
    assert raw_call(fresh, q, r, 5, 7, 0, score_dev=s) == 0 and torch.equal(i32(s), i32(good))
    assert fresh.lib.siggan_verifier_pairs_enable(fresh._h, 5) == 0           # grows; the pack is rebuilt
    assert raw_call(fresh, q, r, 5, 7, 0, best_impostor_dev=bi, score_dev=s) == 0
    assert torch.equal(i32(s), i32(good)) and torch.equal(i32(bi), i32(good.max(dim=1).values))
    fresh.close()

    # E = 1025: the context exists, the pair call is refused at both levels
    wide = SV._Context(DEV, 1025, 2)
    sdw = VC.torch_state(1025)
    wide.bind([p.to(DEV) for k, p in sdw.items() if not k.endswith("num_batches_tracked")], VC.BN_EPS)
    qw = torch.zeros(4, 1025, device=DEV)
    assert wide.lib.siggan_verifier_pairs_enable(wide._h, 4) == _lib.E_ARG
    assert raw_call(wide, qw, qw, 4, 4, 0, score_dev=torch.empty(16, device=DEV)) == _lib.E_ARG
    with pytest.raises(ValueError, match="1024"):
        wide.pairs(qw, None, qw, None, want_matrix=True)
    wide.close()
    assert torch.equal(i32(m.score_matrix(q, r)), i32(good))


# ------------------------------------------------------------------------------------------------------------ 8. evaluation
PARENT_REPORT_KEYS = {"model_metadata", "metrics", "num_test_samples", "genuine_samples", "forgery_samples"}


def test_evaluate_all_pairs_and_the_cli(tmp_path, monkeypatch, capsys):
    e = 128
    m = model_of(e)
    images = VI.gen_x2_bytes(9)
    test_dir = tmp_path / "test"
    for w in range(3):
        (test_dir / f"writer{w}").mkdir(parents=True)
        for k in range(3):
            Image.fromarray(images[3 * w + k]).save(test_dir / f"writer{w}" / f"sig{k}.png")
    res = SV.evaluate_all_pairs(m, test_dir, threshold=0.5)
    assert (res["num_signatures"], res["num_writers"], res["total_pairs"], res["genuine_pairs"], res["impostor_pairs"]) == (9, 3, 36, 9, 27)

    # the same 36 pairs through model(x1, x2), in evaluate_all_pairs' order of files
    ds = SV.SignatureTestDataset.__new__(SV.SignatureTestDataset)
    ds.test_dir, ds.user_signatures = test_dir, {}
    ds._load_signatures()
    paths = [(w, p) for w in ds.user_signatures for p in ds.user_signatures[w]]
    x = torch.from_numpy(np.stack([SV.normalize_uint8(SV.load_uint8(p))[None] for _, p in paths])).to(DEV)
    iu, ju = np.triu_indices(9, 1)
    _, _, sim = m(x[iu], x[ju])
    y_scores = sim.reshape(-1).cpu().numpy().astype(np.float64)
    y_true = np.array([float(paths[i][0] == paths[j][0]) for i, j in zip(iu, ju)])
    want = SV.compute_verification_metrics(y_true, y_scores, (y_scores >= 0.5).astype(int), 0.5)
    got = res["metrics"]
    for k in ("true_positives", "true_negatives", "false_positives", "false_negatives", "total_genuine", "total_forgeries",
              "accuracy", "far", "frr", "precision", "recall", "f1_score", "specificity", "threshold"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["roc_auc_bounds"][0] <= want["roc_auc"] <= got["roc_auc_bounds"][1]
    assert got["eer_bounds"][0] <= want["eer"] <= got["eer_bounds"][1]
    grid = np.unique(np.concatenate([SV.default_threshold_grid(0.5), y_scores.astype(np.float32)]))
    full = SV.evaluate_all_pairs(m, test_dir, threshold=0.5, thresholds=grid)["metrics"]
    for k, v in want.items():
        assert abs(full[k] - v) <= 1e-12, (k, full[k], v)
    # rank-1 and the hardest impostors, from the score matrix
    emb = m.embed_u8(torch.from_numpy(np.stack([SV.load_uint8(p) for _, p in paths])).to(DEV))
    s = m.score_matrix(emb, emb).cpu().numpy()
    wid = np.array([list(ds.user_signatures).index(w) for w, _ in paths])
    gen = wid[:, None] == wid[None, :]
    bg, _, bi, bii = numpy_best(s, gen, ~np.eye(9, dtype=bool))
    assert res["rank1_identification_rate"] == float(np.sum(bg > bi)) / 9
    for wi, w in enumerate(ds.user_signatures):
        rows = np.where(wid == wi)[0]
        rbest = rows[np.argmax(bi[rows])]
        assert res["hardest_impostors"][w]["score"] == float(bi[rbest])
        assert res["hardest_impostors"][w]["impostor"] == str(paths[bii[rbest]][1])
        assert res["hardest_impostors"][w]["impostor_writer"] != w

    # the CLI: --all_pairs adds the object and a block; without it the report and the output are the parent's
    ckpt = tmp_path / "baseline.pth"
    torch.save({"model_state_dict": {k: v.cpu() for k, v in m.state_dict().items()}, "embedding_dim": e}, ckpt)
    monkeypatch.setattr(SV, "_pyplot", lambda: None)                  # the plots are not what this is about
    base = ["signature_verifier_eval", "--baseline_model", str(ckpt), "--test_dir", str(test_dir), "--pairs_per_user", "2"]
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", base + ["--output_dir", str(tmp_path / "plain")])
    SV.main()
    plain_out = capsys.readouterr().out
    monkeypatch.setattr(sys, "argv", base + ["--output_dir", str(tmp_path / "all"), "--all_pairs"])
    SV.main()
    all_out = capsys.readouterr().out
    with open(tmp_path / "plain" / "evaluation_report.json") as f:
        plain = json.load(f)
    with open(tmp_path / "all" / "evaluation_report.json") as f:
        report = json.load(f)
    assert set(plain["models"]["Baseline"]) == PARENT_REPORT_KEYS
    assert set(report["models"]["Baseline"]) == PARENT_REPORT_KEYS | {"all_pairs"}
    assert set(plain) == set(report) == {"evaluation_timestamp", "num_models_evaluated", "models"}
    assert plain["models"]["Baseline"]["metrics"] == report["models"]["Baseline"]["metrics"]
    ap = report["models"]["Baseline"]["all_pairs"]
    assert ap["total_pairs"] == 36 and ap["metrics"]["true_positives"] == want["true_positives"]
    assert ap["metrics"]["far"] == want["far"] and ap["rank1_identification_rate"] == res["rank1_identification_rate"]
    assert "ALL PAIRS" in all_out and "ALL PAIRS" not in plain_out
    assert "Rank-1 identification rate" in all_out
