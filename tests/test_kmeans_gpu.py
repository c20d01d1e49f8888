"""k-means and mode counting on the MI355X (include/siggan_kmeans.h, utils/modes.py) against the numpy yardstick of
kmeanscommon.  Decisions -- labels, seed rows, ``changed``, counts -- are compared exactly, and every case asserts that the
yardstick left none of them undecided (decided by less than twice its derived bound: "pick another seed"), so exact equality
is a sound demand.  Centres are compared bit for bit: given equal labels they are sequential fp64 sums in ascending row order.
The assignment is held to utils.neighbors.knn with k = 1, bit for bit.

Sizes.  The two-level sum takes rows in blocks of 64, the assignment in tiles of 16, the centre update gives a workgroup a
slab of 256 features and walks the labels 64 rows a step, four at a time: n = 15 | 16 | 17 and 63 | 64 | 65 are the two sides of
those boundaries, 67 and 257 leave ragged tails, 1031 and 4099 give 17 and 65 blocks (the fold's threads take a block each up to
256), dim 257 is one feature into a second slab, dim 1024 four full ones; k = 16 | 17 the assignment's tile edge, 256 the limit."""
import ctypes as C
import glob
import json

import numpy as np
import pytest
import torch

import kmeanscommon as K
import verifiercommon as VC
from signature_gan_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
U_NEAR_ONE_SEED = 115082                 # u_0 = 1 - 4.04e-6 (found by a search over 200 000 seeds on the CPU; re-verified below)
PICK_ANOTHER = "the yardstick itself cannot decide this comparison: pick another seed"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def lloyd(x, centres, iterations, mind2=True):
    """The raw call on copies: dict of numpy outputs (centres: after the call)."""
    from signature_gan_amd._call import ptr, stream
    lib = _lib.load()
    xd, cd = dev(x), dev(np.array(centres, dtype=np.float32, copy=True))
    n, dim = x.shape
    k = cd.shape[0]
    size = lib.siggan_kmeans_workspace(n, dim, k)
    assert size > 0
    ws = torch.full((size // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV)       # a dirty workspace
    label = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    md = torch.full((n,), -1.0, dtype=torch.float64, device=DEV) if mind2 else None
    count = torch.full((k,), -7, dtype=torch.int32, device=DEV)
    inertia = torch.full((iterations + 1,), -1.0, dtype=torch.float64, device=DEV)
    changed = torch.full((iterations + 1,), -7, dtype=torch.int32, device=DEV)
    _lib.check(lib.siggan_kmeans_lloyd(xd.device.index or 0, ptr(xd), n, dim, ptr(cd), k, iterations, ptr(label), ptr(md), ptr(count),
                                       ptr(inertia), ptr(changed), ptr(ws), size, stream(xd.device)))
    return dict(centres=cd.cpu().numpy(), labels=label.cpu().numpy(), mind2=None if md is None else md.cpu().numpy(),
                counts=count.cpu().numpy(), inertia=inertia.cpu().numpy(), changed=changed.cpu().numpy())


def knn1(x, centres):
    from signature_gan_amd.utils.neighbors import knn
    d2, index = knn(dev(x), dev(centres), 1)
    return index.cpu().numpy()[:, 0], d2.cpu().numpy()[:, 0]


def other_rows(dim, k):
    """k rows of the normal family that belong to no x the tests use (its n is never 300 + k)."""
    return K.normal(dim, 300 + k)[:k]


# ------------------------------------------------------------------------------------------------------------ assignment
@pytest.mark.parametrize("dim", [1, 4, 5, 40, 128, 1024])
def test_assignment_is_knn_bit_for_bit(dim):
    from signature_gan_amd.utils import modes
    for n in (1, 15, 16, 17, 67, 1031):
        for k in (1, 2, 16, 17, 256):
            if k > n:
                continue
            x, c = K.normal(dim, n), other_rows(dim, k)
            want_label, want_d2 = knn1(x, c)
            cd = dev(c)
            labels, mind2, counts = modes.assign(dev(x), cd)
            assert (labels.dtype, mind2.dtype, counts.dtype) == (torch.int32, torch.float64, torch.int32)
            assert bits(labels.cpu().numpy()) == bits(want_label) and bits(mind2.cpu().numpy()) == bits(want_d2), (n, k)
            assert np.array_equal(counts.cpu().numpy(), np.bincount(want_label, minlength=k))
            assert bits(cd.cpu().numpy()) == bits(c), "iterations = 0 leaves the centres untouched"
            raw = lloyd(x, c, 0, mind2=False)                                        # mind2_dev = NULL: the workspace holds it
            assert bits(raw["labels"]) == bits(want_label) and raw["changed"].tolist() == [n]
            assert raw["inertia"][0] == K.two_level(want_d2)[0], "the two-level sum of the device's own distances, to the bit"
            if n <= 67 or (dim, k) in ((5, 17), (128, 256)):                         # the yardstick: the same decisions
                y_label, y_d2, undecided, bound = K.assign(x, c)
                assert not undecided.any(), PICK_ANOTHER
                assert np.array_equal(y_label, want_label) and np.all(np.abs(y_d2 - want_d2) <= bound)
                assert abs(raw["inertia"][0] - K.inertia(y_d2)) <= K.inertia_bound(bound, y_d2)


@pytest.mark.parametrize("dim,n,k", [(1, 65, 4), (5, 257, 16), (40, 1031, 17), (128, 67, 8)])
def test_lattice_pass_is_bit_equal(dim, n, k):
    """Integer rows against integer centres: every product and sum is exact on both sides, equal distances are plentiful and go
    to the lower centre, and labels, distances and inertia agree to the bit."""
    x = K.lattice(dim, n)
    c = np.concatenate([x[:k // 2], x[:k - k // 2]])                                  # every centre but one twice: exact ties
    out = lloyd(x, c, 0)
    y_label, y_d2, undecided, _ = K.assign(x, c)
    assert not undecided.any()
    assert np.array_equal(out["labels"], y_label) and not np.isin(out["labels"], np.arange(k // 2, 2 * (k // 2))).any()
    assert bits(out["mind2"]) == bits(y_d2) and out["inertia"][0] == K.inertia(y_d2) and out["changed"].tolist() == [n]
    assert np.array_equal(out["counts"], np.bincount(y_label, minlength=k)) and bits(out["centres"]) == bits(c)


# ---------------------------------------------------------------------------------------------------------------- update
def check_update(x, c):
    """One pass from centres c: the labels the update saw are knn's (held to the yardstick), the centres the yardstick's sums."""
    n, k = len(x), len(c)
    label0, _ = knn1(x, c)
    y_label, _, undecided, _ = K.assign(x, c)
    assert not undecided.any(), PICK_ANOTHER
    assert np.array_equal(label0, y_label)
    want, counts0 = K.update(x, label0, c)
    out = lloyd(x, c, 1)
    assert bits(out["centres"]) == bits(want)
    for j in np.flatnonzero(counts0 == 0):
        assert bits(out["centres"][j]) == bits(c[j]), "a centre without rows keeps its bits"
    label1, d2 = knn1(x, want)
    assert bits(out["labels"]) == bits(label1) and bits(out["mind2"]) == bits(d2), "labels and distances belong to the returned centres"
    assert np.array_equal(out["counts"], np.bincount(label1, minlength=k))
    assert out["changed"].tolist() == [n, int((label1 != label0).sum())]
    assert out["inertia"][1] == K.two_level(d2)[0]
    return counts0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1031, 4099])
def test_update_is_the_sequential_sum(n):
    for dim, k in ((5, 3), (40, 17), (257, 2)):
        if k <= n:
            check_update(K.normal(dim, n), other_rows(dim, k))


def test_update_special_centres():
    x = K.normal(5, 257)
    far = np.full((1, 5), 1e3, np.float32)
    # a centre with no row keeps its bits, beside one that takes every row
    counts = check_update(x, np.concatenate([other_rows(5, 1), far]))
    assert counts.tolist() == [257, 0]
    counts = check_update(x, np.concatenate([far, other_rows(5, 2)]))
    assert counts[0] == 0
    # a centre with exactly one row, an outlier: the new centre is a bit copy of that row (x / 1.0)
    lone = x.copy()
    lone[100] += 100.0
    c = np.concatenate([lone[100:101] + 1.0, np.zeros((1, 5), np.float32)])
    assert check_update(lone, c).tolist() == [1, 256]
    assert bits(lloyd(lone, c, 1)["centres"][0]) == bits(lone[100])
    # every row in one centre: k = 1, at a size with a ragged last step, and over several slabs
    assert check_update(K.normal(5, 1031), other_rows(5, 1)).tolist() == [1031]
    assert check_update(K.normal(1024, 67), other_rows(1024, 1)).tolist() == [67]
    # k = n: every row its own centre
    for n in (1, 17, 256):
        x = K.normal(4, n)
        perm = np.random.default_rng(n).permutation(n)
        counts = check_update(x, x[perm])
        assert counts.tolist() == [1] * n
        assert bits(lloyd(x, x[perm], 1)["centres"]) == bits(x[perm])


# ------------------------------------------------------------------------------------------------------------ whole runs
RUNS = [("blobs", dim, n, k) for dim in (5, 128) for n in (257, 1031) for k in (3, 16)] + [("normal", 40, 1031, 17), ("normal", 5, 257, 4)]
PASSES = 12


@pytest.mark.parametrize("family,dim,n,k", RUNS)
def test_whole_runs_pass_by_pass(family, dim, n, k):
    x = K.blobs(dim, n, k)[0] if family == "blobs" else K.normal(dim, n)
    c0 = x[:k].copy()
    c, single, y_prev = c0, [], None
    y_label, _, undecided, _ = K.assign(x, c)
    for t in range(PASSES):
        assert not undecided.any(), PICK_ANOTHER
        want_c, _ = K.update(x, y_label, c)
        y_next, _, undecided, _ = K.assign(x, want_c)
        out = lloyd(x, c, 1)
        assert bits(out["centres"]) == bits(want_c), t
        assert np.array_equal(out["labels"], y_next) and np.array_equal(out["counts"], np.bincount(y_next, minlength=k)), t
        assert out["changed"].tolist() == [n, int((y_next != y_label).sum())], t
        single.append(out)
        c, y_label = want_c, y_next
    assert not undecided.any(), PICK_ANOTHER
    # a 12-pass call equals twelve 1-pass calls, bit for bit
    whole = lloyd(x, c0, PASSES)
    last = single[-1]
    for key in ("centres", "labels", "mind2", "counts"):
        assert bits(whole[key]) == bits(last[key]), key
    assert whole["changed"].tolist() == [n] + [s["changed"][1] for s in single]
    assert bits(whole["inertia"]) == bits(np.array([single[0]["inertia"][0]] + [s["inertia"][1] for s in single]))
    assert np.all(np.diff(whole["inertia"]) <= 0), "Lloyd never raises the inertia (up to rounding: none seen here)"
    # two runs are bit-equal
    again = lloyd(x, c0, PASSES)
    assert all(bits(again[key]) == bits(whole[key]) for key in whole)
    # the fixed point: once changed == 0, further passes change no bit
    still = np.flatnonzero(whole["changed"] == 0)
    if family == "blobs":
        assert still.size, "well-separated blobs converge within 12 passes (checked on the CPU when the test was written)"
    if still.size:
        more = lloyd(x, whole["centres"], 2)
        for key in ("centres", "labels", "mind2", "counts"):
            assert bits(more[key]) == bits(whole[key]), key
        assert more["changed"].tolist() == [n, 0, 0] and more["inertia"].tolist() == [whole["inertia"][-1]] * 3


# --------------------------------------------------------------------------------------------------------------- seeding
def seeded(x, k, seed):
    from signature_gan_amd.utils import modes
    centres, rows = modes.seed_centres(dev(x), k, seed)
    assert (centres.dtype, rows.dtype, tuple(centres.shape), tuple(rows.shape)) == (torch.float32, torch.int32, (k, x.shape[1]), (k,))
    return centres.cpu().numpy(), rows.cpu().numpy()


@pytest.mark.parametrize("seed", [(1 << 32) + 7, 0])
@pytest.mark.parametrize("dim", [5, 128])
def test_seeding_on_the_normal_family(dim, seed):
    for n in (1, 2, 63, 64, 65, 1031):
        for k in (1, 2, 17, 256):
            if k > n:
                continue
            x = K.normal(dim, n)
            want, steps = K.seed_rows(x, k, seed)
            assert K.seeding_is_decided(steps), PICK_ANOTHER
            centres, rows = seeded(x, k, seed)
            assert np.array_equal(rows, want), (n, k)
            assert bits(centres) == bits(x[want]), "centres are bit copies of the chosen rows"
            assert len(set(rows.tolist())) == k, "a chosen row carries no weight"


@pytest.mark.parametrize("dim,n,k", [(1, 65, 17), (5, 257, 40), (40, 1031, 256), (3, 64, 64)])
def test_seeding_on_the_lattice_is_bit_equal(dim, n, k):
    """Integer rows: every m, every prefix and T are exact integers on both sides, so u_s * T and every comparison with it are
    the same bits; duplicate rows (plentiful at dim 1 and 3) carry no weight once one of them is chosen, and when k exceeds the
    number of distinct rows the T == 0 rule takes over."""
    x = K.lattice(dim, n)
    for seed in (0, 9):
        want, steps = K.seed_rows(x, k, seed)
        centres, rows = seeded(x, k, seed)
        assert np.array_equal(rows, want) and bits(centres) == bits(x[want])
    distinct = len({r.tobytes() for r in x})
    if distinct < k:
        assert [st["rule"] for st in steps[distinct:]] == ["unchosen"] * (k - distinct)


def test_seeding_with_fewer_distinct_rows_than_k():
    x = np.repeat(K.lattice(4, 3), 4, axis=0)                                        # 12 rows, 3 distinct
    for seed in (5, 6, 7):
        want, steps = K.seed_rows(x, 8, seed)
        assert [st["rule"] for st in steps[3:]] == ["unchosen"] * 5
        centres, rows = seeded(x, 8, seed)
        assert np.array_equal(rows, want) and bits(centres) == bits(x[want]) and len(set(rows.tolist())) == 8
    # n identical rows: row 0 is drawn, then the lowest rows not chosen
    same = np.ones((70, 5), np.float32)
    _, rows = seeded(same, 70, 3)
    first = min(69, int(np.floor(K.uniform(3, 0) * 70)))
    assert rows.tolist() == [first] + [r for r in range(70) if r != first]


def test_row_zero_at_u_close_to_one():
    u = K.uniform(U_NEAR_ONE_SEED, 0)
    assert 1.0 - 1.0 / 1031 < u < 1.0
    for n in (1, 2, 64, 65, 1031):
        x = K.normal(5, n)
        want, steps = K.seed_rows(x, min(2, n), U_NEAR_ONE_SEED)
        assert want[0] == n - 1 and K.seeding_is_decided(steps)
        _, rows = seeded(x, min(2, n), U_NEAR_ONE_SEED)
        assert np.array_equal(rows, want)


def test_kmeans_restarts_and_result():
    from signature_gan_amd.utils import modes
    x, blob = K.blobs(5, 1031, 16)
    xd = dev(x)
    runs = []
    for r in range(3):                                                               # what restart r must be, from the parts
        centres, rows = modes.seed_centres(xd, 16, 11 + r)
        want_rows, steps = K.seed_rows(x, 16, 11 + r)
        assert K.seeding_is_decided(steps), PICK_ANOTHER
        assert np.array_equal(rows.cpu().numpy(), want_rows)
        runs.append((lloyd(x, centres.cpu().numpy(), 20), want_rows))
    best = int(np.argmin([run["inertia"][-1] for run, _ in runs]))
    res = modes.kmeans(xd, 16, iterations=20, restarts=3, seed=11)
    run, rows = runs[best]
    assert res.restart == best and np.array_equal(res.seed_rows.cpu().numpy(), rows)
    for key, got in (("centres", res.centres), ("labels", res.labels), ("mind2", res.mind2), ("counts", res.counts),
                     ("inertia", res.inertia), ("changed", res.changed)):
        assert bits(got.cpu().numpy()) == bits(run[key]), key
    assert res.empty_clusters == int((run["counts"] == 0).sum())
    one = modes.kmeans(xd, 16, iterations=20, restarts=1, seed=11)
    assert one.restart == 0 and bits(one.centres.cpu().numpy()) == bits(runs[0][0]["centres"])


def test_modes_refusals_on_the_device():
    from signature_gan_amd.utils import modes
    x = dev(K.normal(5, 65))
    for call, text in ((lambda: modes.kmeans(x, 0), r"k = 0 outside \[1, min\(n = 65, 256\)\]"),
                       (lambda: modes.kmeans(x, 66), r"k = 66 outside \[1, min\(n = 65, 256\)\]"),
                       (lambda: modes.kmeans(x, 2.0), "k must be an integer"),
                       (lambda: modes.kmeans(x, 2, iterations=-1), r"iterations = -1 outside \[0, 1000\]"),
                       (lambda: modes.kmeans(x, 2, iterations=1001), r"iterations = 1001 outside \[0, 1000\]"),
                       (lambda: modes.kmeans(x, 2, restarts=0), "restarts must be >= 1"),
                       (lambda: modes.kmeans(x, 2, seed=-1), r"seed = -1 outside \[0, 2\^64\)"),
                       (lambda: modes.kmeans(x.double(), 2), r"x must be float32 \(n >= 1, dim\)"),
                       (lambda: modes.kmeans(x[:0], 1), r"x must be float32 \(n >= 1, dim\)"),
                       (lambda: modes.kmeans(x.t(), 2), "x must be contiguous"),
                       (lambda: modes.kmeans(torch.zeros(2, 1025, device=DEV), 1), r"dim = 1025 outside \[1, 1024\]"),
                       (lambda: modes.kmeans(torch.zeros(65537, 1, device=DEV), 1), "x has 65537 rows, at most 65536"),
                       (lambda: modes.seed_centres(x, 66), "k = 66 outside"),
                       (lambda: modes.assign(x, x[:2, :4].contiguous()), r"centres must be float32 \(1 <= k <= 256, 5\)"),
                       (lambda: modes.assign(x, x[:2].cpu()), "centres must be a tensor on cuda"),
                       (lambda: modes.assign(x[:3], x[:5]), "more than the n = 3 rows"),
                       (lambda: modes.assign(dev(K.normal(2, 300)), dev(K.normal(2, 300))[:257]), "at most 256"),
                       (lambda: modes.mode_coverage(x[:3], x), "at least 4 real rows"),
                       (lambda: modes.mode_coverage(x, x[:, :4].contiguous()), "must share device and dim"),
                       (lambda: modes.mode_coverage(x, x[:2], k=8), "fewer than the k = 8 bins"),
                       (lambda: modes.mode_coverage(x, x, k=40), r"k = 40 outside \[1, min\(n = 33, 256\)\]")):
        with pytest.raises(ValueError, match=text):
            call()


# --------------------------------------------------------------------------------------------------------- mode coverage
MC_DIM, MC_K, MC_REAL, MC_FAKE = 8, 6, 2400, 1500
MC_WEIGHTS = (3, 2, 2, 2, 2, 1)


def test_mode_coverage_on_constructed_sets():
    from signature_gan_amd.utils import modes
    real, real_blob = K.blobs(MC_DIM, MC_REAL, MC_K, weights=MC_WEIGHTS)
    same, _ = K.blobs(MC_DIM, MC_FAKE, MC_K, draw=1, weights=MC_WEIGHTS)
    left_out = 2
    dropped, dropped_blob = K.blobs(MC_DIM, MC_FAKE, MC_K, draw=2, weights=[w if j != left_out else 0 for j, w in enumerate(MC_WEIGHTS)])
    assert not (dropped_blob == left_out).any() and (real_blob == left_out).sum() == 400
    # the yardstick's z-scores for ideal bins put the left-out blob's bin well past the threshold (|z| = 1.96)
    ideal_ref = np.array([300, 200, 200, 200, 200, 100])
    ideal = modes.ndb_from_counts(ideal_ref, np.bincount(dropped_blob, minlength=MC_K))
    assert ideal["z"][left_out] > 10 and ideal["missing_bins"] == [left_out] and left_out in ideal["different_bins"]

    a = modes.mode_coverage(dev(real), dev(same), k=MC_K)
    floor = a["real_holdout_vs_real"]
    assert (a["k"], a["n_bins_rows"], a["n_holdout_rows"], a["n_generated"]) == (MC_K, 1200, 1200, MC_FAKE)
    assert a["converged_at"] is not None and a["empty_clusters"] == [] and a["real_holdout_reason"] is None
    assert floor is not None and a["generated_vs_real"]["ndb_over_k"] <= floor["ndb_over_k"] + 2.0 / MC_K
    assert a["generated_vs_real"]["missing_bins"] == []

    b = modes.mode_coverage(dev(real), dev(dropped), k=MC_K)
    assert b["real_holdout_vs_real"] == floor, "the bins and the floor depend on the real set and the seed alone"
    g = b["generated_vs_real"]
    # which bin is the left-out blob's: the bin its rows of A fall into -- all of them, the blobs are that far apart
    perm = np.random.default_rng(0).permutation(MC_REAL)[:1200]
    bins = modes.kmeans(dev(real[perm]), MC_K, seed=0)
    labels = bins.labels.cpu().numpy()
    (the_bin,) = np.unique(labels[real_blob[perm] == left_out])
    assert np.array_equal(np.unique(labels[real_blob[perm] != left_out]), np.delete(np.arange(MC_K), the_bin)), "k-means found the blobs"
    assert g["missing_bins"] == [int(the_bin)] and int(the_bin) in g["different_bins"] and g["z"][the_bin] > 10
    assert g["js_divergence"] > floor["js_divergence"] and g["ndb_over_k"] > floor["ndb_over_k"]
    assert g["most_under_represented"][0][0] == the_bin
    example = b["under_represented_examples"][0]
    assert example["bin"] == the_bin and real_blob[example["real_row"]] == left_out, "the example is a real row of the missing group"
    # too small a hold-out: the floor is None, with a reason
    few = modes.mode_coverage(dev(real[:9]), dev(same), k=3)
    assert few["real_holdout_vs_real"] is None and "fewer than 2 k = 6" in few["real_holdout_reason"] and few["n_holdout_rows"] == 4


# ------------------------------------------------------------------------------------------------------------------- CLI
LATENT, N, BATCH, SEEDV, SIZE, E, N_REAL = 100, 12, 5, 11, 64, 40, 12


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """The tiny random networks of tests/test_realism_filter_gpu.py (reference_init under a fixed seed, the final conv times
    1024 so that bytes fall on both sides of 128), the E = 40 verifier of verifiercommon, and twelve random real images."""
    from PIL import Image
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=LATENT, output_size=SIZE).to("cuda").eval()
    d = Discriminator(input_size=SIZE).to("cuda").eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
    g._engine.params_changed()
    folder = tmp_path_factory.mktemp("modes_cli")
    ck, vk = folder / "checkpoint.pth", folder / "verifier.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": SIZE}}, ck)
    torch.save({"model_state_dict": VC.torch_state(E), "embedding_dim": E, "epoch": 1}, vk)
    real = folder / "real"
    real.mkdir()
    rng = np.random.default_rng(5)
    for i in range(N_REAL):
        Image.fromarray(rng.integers(0, 256, size=(SIZE, SIZE), dtype=np.uint8), mode="L").save(real / f"r{i:02d}.png")
    return ck, vk, real


def run_evaluate(ck, out, *flags):
    from signature_gan_amd import evaluate_vanilla_gan_signatures as ev
    assert ev.main(["--checkpoint", str(ck), "--n_samples", str(N), "--batch_size", str(BATCH), "--seed", str(SEEDV),
                    "--n_grids", "0", "--output_dir", str(out), *flags]) == 0
    (path,) = glob.glob(str(out / "evaluation_report_*.json"))
    return json.load(open(path))


def scrub(report):
    report = json.loads(json.dumps(report))
    report["metrics"].pop("metrics_computed_at")
    report["evaluation_info"].pop("evaluation_timestamp")
    return report


BLOCK_KEYS = {"k", "n_bins_rows", "n_holdout_rows", "n_generated", "seed", "iterations", "restarts", "restart", "final_inertia",
              "converged_at", "empty_clusters", "generated_vs_real", "real_holdout_vs_real", "real_holdout_reason",
              "under_represented_examples", "feature_space", "feature_dim"}
NDB_KEYS = {"k", "n_ref", "n_test", "alpha", "ndb", "ndb_over_k", "js_divergence", "z", "different_bins", "missing_bins",
            "most_under_represented"}


def test_evaluate_modes(checkpoints, tmp_path, capsys):
    ck, vk, real = checkpoints
    plain = run_evaluate(ck, tmp_path / "p", "--real_dir", str(real))
    plain_text = capsys.readouterr().out
    assert "mode_coverage" not in plain["metrics"] and "ode coverage" not in plain_text
    flagged = run_evaluate(ck, tmp_path / "m", "--real_dir", str(real), "--modes")
    flagged_text = capsys.readouterr().out
    block = flagged["metrics"].pop("mode_coverage")
    assert scrub(flagged) == scrub(plain), "every other key of the report is what it was"

    def comparable(text, out):
        return [line for line in text.replace(str(tmp_path / out), "OUT").splitlines()
                if "ode coverage" not in line and "NDB" not in line and "Missing modes" not in line and "evaluation_report_" not in line]
    assert comparable(flagged_text, "m") == comparable(plain_text, "p"), "and every other printed line"
    added = [line for line in flagged_text.splitlines() if line.startswith(("Mode coverage (NDB): ", "Missing modes: "))]
    assert len(added) == 2, "two summary lines"
    assert set(block) == BLOCK_KEYS and set(block["generated_vs_real"]) == NDB_KEYS == set(block["real_holdout_vs_real"])
    assert (block["feature_space"], block["feature_dim"], block["k"], block["n_bins_rows"], block["n_holdout_rows"],
            block["n_generated"]) == ("pixels/4", 256, 2, 6, 6, N)
    assert block["generated_vs_real"]["n_ref"] == 6 and block["generated_vs_real"]["n_test"] == N
    assert 0.0 <= block["generated_vs_real"]["js_divergence"] <= 1.0
    # K given, and the verifier's embedding space
    three = run_evaluate(ck, tmp_path / "k", "--real_dir", str(real), "--modes", "3")["metrics"]["mode_coverage"]
    assert three["k"] == 3 and len(three["generated_vs_real"]["z"]) == 3
    capsys.readouterr()
    base = ("--real_dir", str(real), "--verifier_checkpoint", str(vk))
    v_plain = run_evaluate(ck, tmp_path / "vp", *base)
    v_flagged = run_evaluate(ck, tmp_path / "vm", *base, "--modes")
    v_block = v_flagged["metrics"].pop("mode_coverage")
    assert scrub(v_flagged) == scrub(v_plain)
    assert (v_block["feature_space"], v_block["feature_dim"], v_block["k"]) == ("verifier", E, 2) and set(v_block) == BLOCK_KEYS
    # the same figures through utils.metrics on the run's own real files
    from signature_gan_amd.data_loader_signatures import SignatureDataset
    from signature_gan_amd.utils import metrics, modes
    ds = SignatureDataset(real)
    real_u8 = torch.from_numpy(np.stack([ds.decode(i, SIZE) for i in range(len(ds))])).to(DEV)
    feats = modes.pixel_features(real_u8)
    again = metrics.calculate_mode_coverage(real_u8, real_u8, k=2)
    assert again["feature_space"] == "pixels/4" and again["k"] == 2
    assert again["real_holdout_vs_real"] == block["real_holdout_vs_real"], "bins and floor depend on the real set alone"
    assert again["final_inertia"] == block["final_inertia"] == modes.kmeans(
        feats[torch.from_numpy(np.random.default_rng(0).permutation(N_REAL)[:6]).to(DEV)].contiguous(), 2, seed=0).inertia[-1].item()

