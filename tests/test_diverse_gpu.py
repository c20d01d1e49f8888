"""Diverse selection on the MI355X (include/siggan_diverse.h, utils.diverse, utils.inference.generate_signatures_diverse) against
the numpy yardstick of diversecommon: order[] exactly, gain2 / min_d2 within B = (dim + 4) * 2^-52 * d2 on the normal family
(every case asserts that the yardstick left no pick undecided, so exact order is a sound demand), bit for bit on the integer
lattice, where all arithmetic is exact and ties are plentiful.

Sizes.  A workgroup owns DIVERSE_ROW_TILE = 32 rows, eight per wave, and 256 threads fold the partials of all workgroups:
n = 31 | 32 | 33, 63 | 64 | 65 and 256 | 257 are the two sides of a row-tile boundary (the last wave ragged, full, one row in a
new workgroup); n = 1, 2 a single ragged wave; n = 8225 is 258 workgroups, where a thread folds a second partial.  dim 1, 4, 5
and 40 leave lanes idle, 128 gives every lane two features, 1024 sixteen and four passes of the LDS staging loop.

The pipeline tests use the tiny networks of tests/test_realism_filter_gpu.py (reference_init under a fixed seed, the two
gains) and the E = 40 verifier of verifiercommon."""
import ctypes as C

import numpy as np
import pytest
import torch

import diversecommon as D
import verifiercommon as VC
from signature_gan_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 256, 257, 1031)
CASES = [(dim, n) for dim in (1, 4, 5, 40, 128) for n in SIZES] + [(1024, n) for n in SIZES if n <= 65] + [(4, 8225)]


def run(x, n_select, eligible=None, anchor_d2=None, first=None, min_separation=0.0):
    from signature_gan_amd.utils.diverse import select_diverse
    order, gain2, count, min_d2 = select_diverse(
        torch.from_numpy(x).to(DEV), n_select, None if eligible is None else torch.from_numpy(eligible).to(DEV),
        None if anchor_d2 is None else torch.from_numpy(anchor_d2).to(DEV), first, min_separation)
    assert (order.dtype, gain2.dtype, count.dtype, min_d2.dtype) == (torch.int32, torch.float64, torch.int32, torch.float64)
    assert tuple(order.shape) == tuple(gain2.shape) == (n_select,) and tuple(count.shape) == (1,) and tuple(min_d2.shape) == (len(x),)
    return order.cpu().numpy(), gain2.cpu().numpy(), int(count.cpu()[0]), min_d2.cpu().numpy()


def close(got, want, dim):
    """Within B where finite; +inf must be +inf."""
    got, want = np.asarray(got), np.asarray(want)
    inf = np.isinf(want)
    return np.array_equal(np.isinf(got), inf) and bool(np.all(np.abs(got[~inf] - want[~inf]) <= D.bound(want[~inf], dim)))


@pytest.mark.parametrize("dim,n", CASES)
def test_normal_family(dim, n):
    x = D.normal(dim, n)
    for n_select in sorted({1, min(40, n), n if n <= 1031 else 40}):
        want_order, want_gain2, want_count, want_min, _, undecided = D.select(x, n_select)
        assert not undecided.any(), "the yardstick itself cannot decide a pick: the case shows nothing"
        order, gain2, count, min_d2 = run(x, n_select)
        assert count == want_count == n_select                          # n_select = n empties the set
        assert np.array_equal(order, want_order)
        assert close(gain2, want_gain2, dim) and close(min_d2, want_min, dim)
        if n_select == n:
            assert sorted(order.tolist()) == list(range(n)) and np.all(min_d2 == 0.0)


@pytest.mark.parametrize("dim", [1, 5, 40])
@pytest.mark.parametrize("n", [2, 33, 257, 1031])
def test_integer_lattice_is_bit_equal(dim, n):
    """Exact arithmetic, many equal values: pins the lowest-row rule and the +inf first pick."""
    x = D.lattice(dim, n)
    for n_select in sorted({1, min(40, n), min(n, 300)}):
        want = D.select(x, n_select)
        order, gain2, count, min_d2 = run(x, n_select)
        assert count == want[2] == n_select and order[0] == 0 and np.isinf(gain2[0])
        assert np.array_equal(order, want[0]) and np.array_equal(gain2, want[1]) and np.array_equal(min_d2, want[3])


def test_duplicates():
    base = D.lattice(5, 30)
    x = np.repeat(base, 3, axis=0)
    distinct = len({r.tobytes() for r in base})
    want = D.select(x, len(x))
    order, gain2, count, min_d2 = run(x, len(x))                         # min_gain2 = 0: duplicates are picked, by flag not value
    assert count == len(x) and np.array_equal(order, want[0]) and np.array_equal(gain2, want[1])
    assert np.all(gain2[distinct:] == 0.0) and np.all(gain2[1:distinct] > 0.0) and sorted(order.tolist()) == list(range(len(x)))
    want = D.select(x, len(x), min_gain2=1e-12)
    order, gain2, count, min_d2 = run(x, len(x), min_separation=1e-6)
    assert count == want[2] == distinct
    assert np.array_equal(order, want[0]) and np.array_equal(gain2, want[1]) and np.array_equal(min_d2, want[3])
    assert np.all(order[count:] == -1) and np.all(gain2[count:] == 0.0) and np.all(min_d2 == 0.0)


def test_masks():
    dim, n = 40, 257
    x = D.normal(dim, n)
    half = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    want = D.select(x, 40, eligible=half)
    assert not want[5].any()
    order, gain2, count, min_d2 = run(x, 40, eligible=half)
    assert count == 40 and np.array_equal(order, want[0]) and np.all(half[order] == 1)
    assert close(gain2, want[1], dim) and close(min_d2, want[3], dim)      # min_d2 covers the ineligible rows too
    # more asked for than the mask holds: the run ends when the eligible rows are used up
    few = np.zeros(n, np.uint8); few[[7, 100, 256]] = 1
    order, gain2, count, _ = run(x, 10, eligible=few)
    assert count == 3 and sorted(order[:3].tolist()) == [7, 100, 256] and order[0] == 7 and np.all(order[3:] == -1) and np.all(gain2[3:] == 0)
    order, gain2, count, min_d2 = run(x, 5, eligible=np.zeros(n, np.uint8))
    assert count == 0 and np.all(order == -1) and np.all(gain2 == 0.0) and np.all(np.isinf(min_d2))
    one = np.zeros(n, np.uint8); one[200] = 1
    order, gain2, count, min_d2 = run(x, 5, eligible=one)
    assert count == 1 and order[0] == 200 and np.isinf(gain2[0]) and min_d2[200] == 0.0
    assert close(min_d2, D.d2_to_row(x.astype(np.float64), 200), dim)


def test_anchors_and_min_gain():
    from signature_gan_amd.utils.neighbors import knn
    dim, n = 40, 257
    x, other = D.normal(dim, n), D.normal(dim, 65) * 0.5
    anchor = knn(torch.from_numpy(x).to(DEV), torch.from_numpy(other).to(DEV), 1)[0][:, 0].contiguous().cpu().numpy()
    want = D.select(x, 40, anchor_d2=anchor)
    assert not want[5].any()
    order, gain2, count, min_d2 = run(x, 40, anchor_d2=anchor)
    assert count == 40 and np.array_equal(order, want[0]) and order[0] == int(np.argmax(anchor)) and gain2[0] == anchor.max()
    assert close(gain2, want[1], dim) and close(min_d2, want[3], dim) and np.all(min_d2 <= anchor)
    # pick 0 obeys min_gain2: nothing is as far from the anchors as asked
    order, gain2, count, min_d2 = run(x, 40, anchor_d2=anchor, min_separation=float(np.sqrt(anchor.max())) * 1.01)
    assert count == 0 and np.all(order == -1) and np.array_equal(min_d2, anchor)
    # a separation in between stops the run where the yardstick stops
    sep = float(np.sqrt(want[1][20] * 1.0001))
    want = D.select(x, 40, anchor_d2=anchor, min_gain2=sep * sep)
    order, gain2, count, _ = run(x, 40, anchor_d2=anchor, min_separation=sep)
    assert 0 < count == want[2] < 40 and np.array_equal(order, want[0]) and np.all(gain2[count:] == 0.0)


def test_forced_first_is_taken_as_given():
    dim, n = 5, 65
    x = D.normal(dim, n)
    mask = np.ones(n, np.uint8); mask[40] = 0
    want = D.select(x, 10, eligible=mask, first=40)
    assert not want[5].any()
    order, gain2, count, min_d2 = run(x, 10, eligible=mask, first=40)
    assert count == 10 and order[0] == 40 and np.isinf(gain2[0]) and np.array_equal(order, want[0]) and close(gain2, want[1], dim)
    # min_gain2 does not apply to it either, and with an all-zero mask it is the only pick
    anchor = np.full(n, 0.25)
    order, gain2, count, _ = run(x, 10, eligible=np.zeros(n, np.uint8), anchor_d2=anchor, first=3, min_separation=10.0)
    assert count == 1 and order[0] == 3 and gain2[0] == 0.25 and np.all(order[1:] == -1)


@pytest.mark.parametrize("dim,n", [(5, 257), (128, 1031)])
def test_picks_are_greedy_by_replay(dim, n):
    """Independent of the yardstick's order: replay m along the DEVICE's picks; every gain is that row's own value within B
    and the largest eligible value within B.  With q the replay's best row and p the device's pick: replay m[q] <= device
    m[q] + B <= gain + B, and replay m[q] >= replay m[p] >= gain - B."""
    x = D.normal(dim, n)
    mask = (np.random.default_rng(9).random(n) < 0.7).astype(np.uint8)
    order, gain2, count, min_d2 = run(x, 60, eligible=mask)
    assert count == 60 and len(set(order.tolist())) == 60
    pairs, final = D.replay(x, order, count, eligible=mask)
    for t, (own, best) in enumerate(pairs):
        if np.isinf(best):
            assert np.isinf(gain2[t])
            continue
        assert abs(gain2[t] - own) <= D.bound(own, dim) and abs(gain2[t] - best) <= D.bound(best, dim), t
    assert close(min_d2, final, dim)


def test_guards_survive_and_min_d2_may_be_null():
    dim, n, n_select, g = 40, 257, 40, 16
    x = torch.from_numpy(D.normal(dim, n)).to(DEV)
    lib = _lib.load()
    size = lib.siggan_select_diverse_workspace(n)
    ws = torch.full((size // 8 + 1 + 2 * g,), float("nan"), dtype=torch.float64, device=DEV)
    order = torch.full((n_select + 2 * g,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    gain2 = torch.full((n_select + 2 * g,), -777.0, dtype=torch.float64, device=DEV)
    count = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    min_d2 = torch.full((n + 2 * g,), -777.0, dtype=torch.float64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off * t.element_size())          # noqa: E731
    want = D.select(x.cpu().numpy(), n_select)
    for with_min in (True, False):
        order[g:-g] = 0x5A5A5A5A
        _lib.check(lib.siggan_select_diverse(0, p(x), n, dim, None, None, -1, n_select, 0.0, p(order, g), p(gain2, g), p(count, 1),
                                             p(min_d2, g) if with_min else None, p(ws, g), size, stream))
        o, g2, c, m, w = order.cpu().numpy(), gain2.cpu().numpy(), count.cpu().numpy(), min_d2.cpu().numpy(), ws.cpu().numpy()
        assert np.all(o[:g] == 0x5A5A5A5A) and np.all(o[-g:] == 0x5A5A5A5A) and np.array_equal(o[g:-g], want[0])
        assert np.all(g2[:g] == -777.0) and np.all(g2[-g:] == -777.0) and close(g2[g:-g], want[1], dim)
        assert c.tolist() == [0x5A5A5A5A, n_select, 0x5A5A5A5A]
        assert np.all(m[:g] == -777.0) and np.all(m[-g:] == -777.0) and close(m[g:-g], want[3], dim)
        assert np.all(np.isnan(w[:g])) and np.all(np.isnan(w[g + size // 8 + 1:]))  # the workspace is used inside its size only


def test_runs_and_streams_are_bit_equal():
    dim, n = 128, 1031
    x = D.normal(dim, n)
    mask = (np.random.default_rng(3).random(n) < 0.8).astype(np.uint8)
    a = run(x, 100, eligible=mask)
    b = run(x, 100, eligible=mask)
    streams = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            streams.append(run(x, 100, eligible=mask))
    for other in (b, *streams):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2] and np.array_equal(a[3], other[3])


def test_wrapper_argument_checks():
    from signature_gan_amd.utils.diverse import eligibility, select_diverse
    x = torch.zeros(9, 8, device=DEV)
    for bad in (dict(n_select=0), dict(n_select=10), dict(n_select=3, first=9), dict(n_select=3, first=-2),
                dict(n_select=3, min_separation=-1.0), dict(n_select=3, min_separation=float("nan")),
                dict(n_select=3, eligible=torch.zeros(9, device=DEV)), dict(n_select=3, eligible=torch.zeros(8, dtype=torch.uint8, device=DEV)),
                dict(n_select=3, anchor_d2=torch.zeros(9, device=DEV)), dict(n_select=3, anchor_d2=torch.zeros(9, dtype=torch.float64))):
        with pytest.raises(ValueError):
            select_diverse(x, **bad)
    for bad_x in (x.double(), x[:, ::2], x[0], x.cpu()):
        with pytest.raises(ValueError):
            select_diverse(bad_x, 3)
    for bad_scores in (torch.zeros(6), torch.zeros(6, dtype=torch.float64, device=DEV), torch.zeros(2, 3, device=DEV),
                       torch.zeros(12, device=DEV)[::2], torch.zeros(0, device=DEV), [0.5, 0.1]):
        with pytest.raises(ValueError, match="scores must be"):
            eligibility(bad_scores, 0.5)
    scores = torch.tensor([0.5, 0.9, 0.5, 0.1, 0.5, 0.7], device=DEV)
    for bad_ratio in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="keep_ratio"):
            eligibility(scores, bad_ratio)
    with pytest.raises(ValueError, match="come together"):
        eligibility(scores, 0.5, nearest_real_d2=torch.zeros(6, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="come together"):
        eligibility(scores, 0.5, floor2=1.0)
    assert eligibility(scores, 0.5).cpu().tolist() == [1, 1, 0, 0, 0, 1]              # ties as select_topk resolves them
    assert eligibility(scores, 0.51).cpu().tolist() == [1, 1, 1, 0, 0, 1]             # ceil(0.51 * 6) = 4
    d2 = torch.tensor([4.0, 0.5, 4.0, 4.0, 4.0, 1.0], dtype=torch.float64, device=DEV)
    assert eligibility(scores, 0.5, d2, 1.0).cpu().tolist() == [1, 0, 0, 0, 0, 1]     # >= floor2 stays
    assert eligibility(scores, 1.0, d2, torch.tensor(1.5, dtype=torch.float64, device=DEV)).cpu().tolist() == [1, 0, 1, 1, 1, 0]


# ---- the pipeline -----------------------------------------------------------------------------------------------------------
N, RATIO, BATCH, LATENT, SEEDV, E = 8, 4.0, 16, 100, 1234, 40


@pytest.fixture(scope="module")
def nets():
    from signature_gan_amd import signature_verifier_eval as SV
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=LATENT, output_size=64).to(DEV).eval()
    d = Discriminator(input_size=64).to(DEV).eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
        d.state_dict()["classifier.0.weight"].mul_(1024.0)
    g._engine.params_changed(); d._engine.params_changed()
    v = SV.SiameseNetwork(E, max_images=16)                                # 32 pool images: two embedding chunks
    v.load_state_dict(VC.torch_state(E), strict=True)
    return g, d, v.to(DEV).eval()


def diverse(nets, **kw):
    from signature_gan_amd.utils.inference import generate_signatures_diverse
    g, d, v = nets
    args = dict(seed=SEEDV, batch_size=BATCH, oversampling_ratio=RATIO)
    args.update(kw)
    return generate_signatures_diverse(g, d, v, N, LATENT, torch.device(DEV), **args)


@pytest.mark.parametrize("threshold", [None, 127])
def test_pipeline_with_exactly_n_eligible_is_the_filter_set(nets, threshold):
    from signature_gan_amd.utils.inference import generate_signatures_filtered
    g, d, _ = nets
    images, scores, report = diverse(nets, keep_ratio=0.25, threshold=threshold)
    f_images, f_scores = generate_signatures_filtered(g, d, N, LATENT, torch.device(DEV), seed=SEEDV, batch_size=BATCH,
                                                      oversampling_ratio=RATIO, threshold=threshold)
    assert len(images) == len(f_images) == N and (report["pool"], report["eligible"], report["selected"]) == (32, N, N)
    assert report["stopped_by"] == "count" and len(set(f_scores)) == N
    got = {s: np.array(im).tobytes() for im, s in zip(images, scores)}
    want = {s: np.array(im).tobytes() for im, s in zip(f_images, f_scores)}
    assert got == want                                                     # the same set: every image's bytes and score
    assert scores[0] == f_scores[0]                                        # the first pick is the most realistic
    assert report["diverse"]["mean_realism"] == pytest.approx(report["top_n"]["mean_realism"], rel=1e-12)
    assert report["diverse"]["min_nn_distance"] == pytest.approx(report["top_n"]["min_nn_distance"], rel=1e-9)
    if threshold is not None:
        assert all(set(np.unique(np.array(im))) <= {0, 255} for im in images)


def test_pipeline_picks_are_select_diverse_on_the_returned_pool(nets):
    from signature_gan_amd.utils.diverse import diversity_summary, select_diverse
    from signature_gan_amd.utils.neighbors import knn
    _, _, v = nets
    images, scores, report = diverse(nets, keep_ratio=1.0, return_pool=True)
    dev = report.pop("_device")
    pool, pool_scores, emb, mask = dev["pool"], dev["scores"], dev["embeddings"], dev["eligible"]
    assert tuple(pool.shape) == (32, 64, 64) and tuple(emb.shape) == (32, E) and mask.cpu().tolist() == [1] * 32
    assert torch.equal(emb, torch.cat([v.embed_u8(pool[:16]), v.embed_u8(pool[16:])]))
    first = int(torch.argmax(pool_scores))
    order, gain2, count, min_d2 = select_diverse(emb, N, mask, None, first, 0.0)
    order_h = order.cpu().numpy()
    assert [p["pool_index"] for p in report["picks"]] == order_h.tolist() and order_h[0] == first and int(count.cpu()) == N
    want = D.select(emb.cpu().numpy(), N, first=first)
    assert np.array_equal(order_h, want[0]) or want[5].any()
    for im, s, p in zip(images, scores, order_h):
        assert np.array_equal(np.array(im), pool[p].cpu().numpy()) and s == float(pool_scores[p])
    sel, top = emb[order.long()].contiguous(), emb[torch.argsort(pool_scores, descending=True, stable=True)[:N]].contiguous()
    top_scores = np.sort(pool_scores.cpu().numpy())[::-1][:N]
    summary = diversity_summary(32, 32, N, order_h, gain2.cpu().numpy(), N, pool_scores[order.long()].cpu().numpy(), None,
                                float(min_d2.max().cpu()), knn(sel, sel, 1, exclude_self=True)[0][:, 0].cpu().numpy(), top_scores,
                                knn(top, top, 1, exclude_self=True)[0][:, 0].cpu().numpy())
    assert report == summary
    assert report["picks"][0]["gain"] is None and all(p["gain"] > 0 and p["nearest_real"] is None for p in report["picks"][1:])
    print(report["diverse"], report["top_n"])
    # farthest-first traversal from any start is within a factor 2 of the best possible smallest distance among N rows
    # (Gonzalez 1985), and with every row eligible the top-n is one such choice; no choice of N rows has a higher mean score
    assert report["diverse"]["min_nn_distance"] >= 0.5 * report["top_n"]["min_nn_distance"]
    assert report["diverse"]["mean_realism"] <= report["top_n"]["mean_realism"] * (1 + 1e-12)


def test_pipeline_excludes_a_planted_copy_of_a_real_signature(nets):
    _, _, report = diverse(nets, keep_ratio=1.0, return_pool=True)
    pool = report["_device"]["pool"]
    victim = report["picks"][1]["pool_index"]                              # a row the unconstrained run does pick
    rng = np.random.default_rng(11)
    real = rng.integers(0, 256, size=(6, 64, 64), dtype=np.uint8)
    real[2] = pool[victim].cpu().numpy()                                   # a real signature the Generator "memorised"
    images, scores, rep = diverse(nets, keep_ratio=1.0, real_u8=real, memorisation_ratio=0.01, return_pool=True)
    mask = rep["_device"]["eligible"].cpu().numpy()
    assert mask[victim] == 0 and rep["eligible"] == int(mask.sum()) and victim not in [p["pool_index"] for p in rep["picks"]]
    assert all(p["nearest_real"] > 0 and mask[p["pool_index"]] == 1 for p in rep["picks"]) and len(images) == rep["selected"] >= 1
    with pytest.raises(ValueError, match="come together"):
        diverse(nets, real_u8=real)
    with pytest.raises(ValueError, match="come together"):
        diverse(nets, memorisation_ratio=0.5)


def test_pipeline_refuses_where_the_filter_falls_back(nets):
    g, _, _ = nets
    g.train()
    try:
        with pytest.raises(ValueError, match="no host route"):
            diverse(nets)
    finally:
        g.eval()
    with pytest.raises(ValueError, match="no host route"):
        diverse(nets, oversampling_ratio=(_lib.SELECT_MAX + 8) / N)
