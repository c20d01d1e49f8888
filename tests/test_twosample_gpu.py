"""siggan_kernel_forms on the MI355X (include/siggan_twosample.h, csrc/twosample.hip, utils/twosample.py), through the C ABI
and the Python wrappers, and the two statistics made of it end to end, down to ``evaluate_vanilla_gan_signatures
--verifier_kid``.

Yardstick: tests/twosamplecommon.py, numpy fp64 on the same fp32 inputs -- K from direct sums, the diagonal zeroed by
position, the forms as (A * (K0 @ A)).sum(0).  Two kinds of check:

* integer data (entries in {-2 .. 2}, polynomial kernel with integer gamma and coef0): every kernel value and every partial
  sum is an integer far below 2^53 (the largest form here is below 2^42), so forms and diag must equal the yardstick BIT FOR
  BIT whatever order either side sums in.  This is what proves the chained MFMA operand mapping: any slip moves integers.
* float data: per form the bound B_form derived in twosamplecommon's docstring (exact products; gamma_dim on the dot product
  or on each of the three sums of d2; the propagation through the cube or through exp, |dk| <= k (gamma B_ij + |arg| U + the
  library's 1 ulp); gamma_terms on the outer sum of |k|), not tuned; each case prints worst error / bound.

Shapes are the smallest at which something can go wrong.  dim 1 (inside one K step), 4 (one step), 5 (a step and a tail), 40
(two and a half 16-feature chunks, 16-byte loads), 128 (the verifier's size); n 1, 2, 15, 16, 17 (a partial tile, a full one,
a tail), 33 (a second row block of one partial tile), 67 and 131 (three and five row blocks, nine j-tiles over four waves with
a ragged end); cols 1, 16, 17, 65 (byte-wise label loads, a partial sub-tile, a second wave) and 20, 257 (4-byte label loads;
a second column chunk of one column).  Measured margins: profiles/twosample_parity_margins.json."""
import ctypes as C
import glob
import json

import numpy as np
import pytest
import torch

import twosamplecommon as TC
import verifiercommon as VC
import signature_gan_amd                                              # noqa: F401
from signature_gan_amd import _lib
from signature_gan_amd.utils import twosample as TS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def raw_forms(xd, ld, kind, gamma, coef0=1.0, degree=3, n=None, dim=None, cols=None, ws=None, ws_bytes=None, forms=None, diag=None,
              stream=None):
    """The C call itself -> return code; sizes default to the tensors', the workspace to a fresh one of the stated size."""
    lib = _lib.load()
    n = xd.shape[0] if n is None else n
    dim = xd.shape[1] if dim is None else dim
    cols = ld.shape[1] if cols is None else cols
    size = lib.siggan_kernel_forms_workspace(n, cols)
    if ws is None:
        ws = torch.empty(max(size, 8) // 8, dtype=torch.float64, device=DEV)
    spec = _lib.KernelSpec(TS.KINDS[kind], degree, gamma, coef0)
    return lib.siggan_kernel_forms(0, p(xd), n, dim, C.byref(spec), p(ld), cols, p(forms), p(diag), p(ws), size if ws_bytes is None else ws_bytes,
                                   stream)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.int64), (want + 0.0).view(np.int64)), f"{what}: differs at {np.argwhere(got != want)[:4].tolist()}"


INTEGER_CASES = [  # (dim, n, cols)
    (1, 1, 1), (1, 2, 16), (1, 17, 17), (4, 15, 1), (4, 16, 65), (4, 131, 17), (5, 2, 17), (5, 17, 16), (5, 67, 65), (40, 16, 17),
    (40, 33, 20), (40, 131, 65), (40, 67, 257), (128, 15, 16), (128, 17, 1), (128, 131, 65), (128, 67, 20),
]


@pytest.mark.parametrize("dim,n,cols", INTEGER_CASES)
def test_integer_data_is_exact(dim, n, cols):
    x, labels = TC.integer_rows(n, dim), TC.random_labels(n, cols)
    xd, ld = dev(x), dev(labels)
    for degree, coef0 in ((3, 0.0), (1, 1.0), (2, 1.0)):
        want, _, want_diag = TC.forms(x, labels, "poly", 1.0, coef0, degree)
        assert np.abs(want).max() < 2.0 ** 53 and np.array_equal(want, np.round(want))
        got, diag = TS.kernel_forms(xd, ld, kind="poly", gamma=1.0, coef0=coef0, degree=degree, want_diag=True)
        assert_bit_equal(got.cpu().numpy(), want, f"forms dim={dim} n={n} cols={cols} degree={degree}")
        assert_bit_equal(diag.cpu().numpy(), want_diag, f"diag dim={dim} n={n} cols={cols} degree={degree}")
        assert_bit_equal(TS.kernel_forms(xd, ld, kind="poly", gamma=1.0, coef0=coef0, degree=degree).cpu().numpy(), want, "without diag")


def test_label_edge_cases():
    n, dim = 67, 40
    x = TC.integer_rows(n, dim, seed=1)
    x[41] = x[7]                                                          # two bit-identical rows, in different tiles
    k, _ = TC.kernel_matrix(x, "poly", 1.0, 0.0, 3)
    k0 = k.copy()
    np.fill_diagonal(k0, 0.0)
    base = TC.random_labels(n, 1, seed=2)[:, 0]
    cols = {
        "all zero": np.zeros(n, np.uint8),
        "one row in A": np.eye(1, n, 7, dtype=np.uint8)[0],
        "two identical rows in A": np.eye(1, n, 7, dtype=np.uint8)[0] + np.eye(1, n, 41, dtype=np.uint8)[0],
        "every row in A": np.ones(n, np.uint8),
        "random": base,
        "random, 0 written as 3 and 255": np.where(base == 0, np.where(np.arange(n) % 2 == 0, 3, 255), base).astype(np.uint8),
        "random, A and B swapped": np.where(base == 1, 2, np.where(base == 2, 1, 0)).astype(np.uint8),
    }
    labels = np.stack(list(cols.values()), axis=1)
    want, _, _ = TC.forms(x, labels, "poly", 1.0, 0.0, 3)
    got = TS.kernel_forms(dev(x), dev(labels), kind="poly", gamma=1.0, coef0=0.0, degree=3).cpu().numpy()
    assert_bit_equal(got, want, "label edge cases")
    f = dict(zip(cols, got))
    assert not f["all zero"].any()
    assert not f["one row in A"].any()                                    # the diagonal is excluded by row number
    assert f["two identical rows in A"][0] == 2.0 * k[7, 7] > 0 and not f["two identical rows in A"][1:].any()   # not by value
    assert f["every row in A"][0] == k0.sum() and not f["every row in A"][1:].any()
    assert np.array_equal(f["random, 0 written as 3 and 255"], f["random"])
    assert np.array_equal(f["random, A and B swapped"], f["random"][[1, 0, 2]])


FLOAT_CASES = [(5, 67, 17), (40, 131, 65), (128, 131, 16), (128, 17, 20), (4, 33, 1)]


@pytest.mark.parametrize("kind", ["poly", "rbf"])
@pytest.mark.parametrize("family", ["normal", "unit"])
@pytest.mark.parametrize("dim,n,cols", FLOAT_CASES)
def test_float_data_within_the_derived_bound(dim, n, cols, family, kind):
    x, labels = TC.float_rows(family, n, dim), TC.random_labels(n, cols, seed=3)
    gamma = 1.0 / dim if kind == "poly" else TC.median_gamma(x)
    want, bound, want_diag = TC.forms(x, labels, kind, gamma, 1.0, 3)
    got, diag = TS.kernel_forms(dev(x), dev(labels), kind=kind, gamma=gamma, coef0=1.0, degree=3, want_diag=True)
    got, diag = got.cpu().numpy(), diag.cpu().numpy()
    err = np.abs(got - want)
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print(f"MARGIN {kind} {family} dim={dim} n={n} cols={cols}: worst form error / bound {ratio:.3e} "
          f"(largest bound / |form| {float((bound[live] / np.abs(want[live])).max()) if live.any() else 0.0:.3e})")
    assert (err <= bound).all(), f"forms off at {np.argwhere(err > bound)[:4].tolist()}"
    if kind == "rbf":
        assert (diag == 1.0).all()                                        # d2 of a row against itself is exactly 0
    else:
        _, bk = TC.kernel_matrix(x, kind, gamma, 1.0, 3)
        assert (np.abs(diag - want_diag) <= np.diagonal(bk)).all()


def test_equal_bits_run_to_run_on_another_stream_and_over_a_dirty_workspace():
    x, labels = TC.float_rows("unit", 131, 128, seed=4), TC.random_labels(131, 65, seed=4)
    xd, ld = dev(x), dev(labels)
    gamma = TC.median_gamma(x)
    first = TS.kernel_forms(xd, ld, kind="rbf", gamma=gamma, want_diag=True)
    second = TS.kernel_forms(xd, ld, kind="rbf", gamma=gamma, want_diag=True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(torch.device(DEV)))
    with torch.cuda.stream(side):
        third = TS.kernel_forms(xd, ld, kind="rbf", gamma=gamma, want_diag=True)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, third))
    size = _lib.load().siggan_kernel_forms_workspace(131, 65)
    assert size == 24 * 5 * 65 + 8 * 131                                  # ceil(131 / 32) row blocks of partial forms, then the norms
    for fill in (float("nan"), 1e300):
        ws = torch.full((size // 8 + 1,), fill, dtype=torch.float64, device=DEV)
        forms = torch.empty(65, 3, dtype=torch.float64, device=DEV)
        diag = torch.empty(131, dtype=torch.float64, device=DEV)
        assert raw_forms(xd, ld, "rbf", gamma, ws=ws, forms=forms, diag=diag) == 0
        torch.cuda.synchronize()
        assert torch.equal(forms, first[0]) and torch.equal(diag, first[1])
        assert bool(torch.isnan(ws[-1])) or float(ws[-1]) == fill          # nothing written past the stated size


def test_columns_beyond_the_maximum_go_in_chunks():
    n, cols = 17, _lib.TWOSAMPLE_MAX_COLS + 3
    x, labels = TC.integer_rows(n, 4, seed=5), TC.random_labels(n, cols, seed=5)
    want, _, _ = TC.forms(x, labels, "poly", 1.0, 1.0, 2)
    got = TS.kernel_forms(dev(x), dev(labels), kind="poly", gamma=1.0, coef0=1.0, degree=2)
    assert_bit_equal(got.cpu().numpy(), want, "chunked columns")


def test_refusals_launch_nothing():
    lib = _lib.load()
    x, labels = TC.integer_rows(9, 8, seed=6), TC.random_labels(9, 5, seed=6)
    xd, ld = dev(x), dev(labels)
    forms = torch.full((5, 3), -1.0, dtype=torch.float64, device=DEV)
    diag = torch.full((9,), -1.0, dtype=torch.float64, device=DEV)
    out = dict(forms=forms, diag=diag)
    size = lib.siggan_kernel_forms_workspace(9, 5)
    bad = [(dict(n=0), b"n ="), (dict(cols=0), b"cols ="), (dict(dim=0), b"dim"),
           (dict(n=_lib.TWOSAMPLE_MAX_N + 1), b"n ="), (dict(cols=_lib.TWOSAMPLE_MAX_COLS + 1), b"cols ="),
           (dict(dim=_lib.TWOSAMPLE_MAX_DIM + 1), b"dim"), (dict(degree=0), b"degree"), (dict(degree=4), b"degree"),
           (dict(gamma=0.0), b"gamma"), (dict(gamma=-1.0), b"gamma"), (dict(gamma=float("nan")), b"gamma"),
           (dict(gamma=float("inf")), b"gamma"), (dict(coef0=float("nan")), b"coef0"), (dict(ws_bytes=size - 1), b"workspace")]
    for kw, word in bad:
        args = dict(kind="poly", gamma=1.0, ws=torch.empty(64, dtype=torch.float64, device=DEV), **out)
        args.update(kw)
        assert raw_forms(xd, ld, **args) == _lib.E_ARG, kw
        assert word in lib.siggan_last_error(), (kw, lib.siggan_last_error())
        with pytest.raises(ValueError, match="siggan_kernel_forms"):
            _lib.check(_lib.E_ARG)
    assert lib.siggan_kernel_forms_workspace(0, 5) == 0 and lib.siggan_kernel_forms_workspace(9, _lib.TWOSAMPLE_MAX_COLS + 1) == 0
    torch.cuda.synchronize()
    assert (forms == -1).all() and (diag == -1).all()
    assert raw_forms(xd, ld, "poly", 1.0, **out) == 0 and raw_forms(xd, ld, "rbf", 1.0, degree=0, **out) == 0   # RBF ignores degree
    torch.cuda.synchronize()
    assert (forms != -1).all()
    # the wrapper: its own checks, and the library's message as ValueError
    for kw in (dict(degree=0), dict(degree=4), dict(gamma=0.0), dict(gamma=float("nan"))):
        with pytest.raises(ValueError, match="siggan_kernel_forms"):
            TS.kernel_forms(xd, ld, **{**dict(kind="poly", gamma=1.0), **kw})
    with pytest.raises(ValueError, match="n = 0"):
        TS.kernel_forms(xd[:0], ld[:0], kind="poly", gamma=1.0)
    with pytest.raises(ValueError, match="cols = 0"):
        TS.kernel_forms(xd, ld[:, :0].contiguous(), kind="poly", gamma=1.0)
    with pytest.raises(ValueError, match="dim 0"):
        TS.kernel_forms(xd[:, :0].contiguous(), ld, kind="poly", gamma=1.0)
    with pytest.raises(ValueError, match="MAX_N"):
        TS.kernel_forms(torch.zeros(_lib.TWOSAMPLE_MAX_N + 1, 1, device=DEV), torch.zeros(_lib.TWOSAMPLE_MAX_N + 1, 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="dim 1025"):
        TS.kernel_forms(torch.zeros(9, _lib.TWOSAMPLE_MAX_DIM + 1, device=DEV), ld, kind="poly", gamma=1.0)
    for bad_x, bad_l in ((xd, ld.cpu()), (xd, ld.to(torch.int8)), (xd, ld.to(torch.int32)), (xd, ld[:8]), (xd, ld[:, ::2]), (xd.cpu(), ld),
                         (xd.double(), ld), (xd.t().contiguous().t(), ld), (xd, ld.reshape(-1))):
        with pytest.raises(ValueError):
            TS.kernel_forms(bad_x, bad_l, kind="poly", gamma=1.0)
    with pytest.raises(ValueError, match="kind"):
        TS.kernel_forms(xd, ld, kind="linear", gamma=1.0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            TS.kernel_forms(xd, ld.to("cuda:1"), kind="poly", gamma=1.0)


N_REAL, N_FAKE, DIM, PERMS = 64, 48, 8, 199


def two_sets(seed, shift):
    rng = np.random.default_rng(seed)
    real = rng.standard_normal((N_REAL, DIM)).astype(np.float32)
    fake = (rng.standard_normal((N_FAKE, DIM)) + shift).astype(np.float32)
    return real, fake


@pytest.mark.parametrize("shift", [0.0, 1.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_permutation_test_and_kid_end_to_end(seed, shift):
    """The observed MMD^2 and every permuted one within the bound propagated from the forms (twosamplecommon.mmd2); the p-value
    EXACTLY, which is sound because no permuted statistic of the yardstick lies within 2 x bound of the observed one (asserted
    first; the gaps are about 1e-5 against bounds of about 1e-13).  With the generated set shifted by +1.0 per coordinate p is
    the minimum 1 / 200; with both sets from one distribution the yardstick gives p = 0.155, 0.26 and 0.11 for seeds 0, 1, 2."""
    real, fake = two_sets(seed, shift)
    pooled = np.concatenate([real, fake])
    rd, fd = dev(real), dev(fake)
    stats, gamma = TS.permutation_stats(rd, fd, PERMS, "rbf", None, seed)
    assert gamma == pytest.approx(TC.median_gamma(pooled), rel=1e-14)
    labels = TS.permutation_labels(N_REAL, N_FAKE, PERMS, seed)
    want, bound = TC.mmd2(*TC.forms(pooled, labels, "rbf", gamma)[:2], N_REAL, N_FAKE)
    gap, need = np.abs(want[1:] - want[0]), 2 * np.maximum(bound[1:], bound[0])
    assert (gap > need).all(), f"seed {seed}: the yardstick leaves {int((gap <= need).sum())} comparisons undecided; pick another seed"
    err = np.abs(stats - want)
    print(f"MARGIN mmd2 seed={seed} shift={shift}: worst error / bound {float((err / bound).max()):.3e}, smallest gap {gap.min():.3e} "
          f"against bound {bound.max():.3e}")
    assert (err <= bound).all()
    p_want = (1 + int((want[1:] >= want[0]).sum())) / (1 + PERMS)
    out = TS.mmd_permutation_test(rd, fd, permutations=PERMS, seed=seed)
    assert set(out) == {"mmd2", "p_value", "null_mean", "null_std", "null_q95", "permutations", "kind", "gamma"}
    assert out["p_value"] == p_want and out["mmd2"] == stats[0] and out["gamma"] == gamma and out["kind"] == "rbf"
    assert out["null_mean"] == float(np.mean(stats[1:])) and out["null_q95"] == float(np.quantile(stats[1:], 0.95))
    print(f"seed {seed} shift {shift}: mmd2 {out['mmd2']:.6f}, p = {out['p_value']}")
    if shift:
        assert out["p_value"] == 1 / 200
    else:
        assert out["p_value"] == {0: 0.155, 1: 0.26, 2: 0.11}[seed]        # what the yardstick gives on the CPU for these draws

    subsets, size = 20, 32
    values, full, got_size, kgamma = TS.kid_values(rd, fd, subsets, size, None, seed)
    assert (got_size, kgamma) == (size, 1.0 / DIM)
    f, b, _ = TC.forms(pooled, TS.subset_labels(N_REAL, N_FAKE, subsets, size, seed), "poly", kgamma, 1.0, 3)
    want_v, bound_v = TC.mmd2(f, b, size, size)
    f, b, _ = TC.forms(pooled, labels[:, :1], "poly", kgamma, 1.0, 3)
    want_full, bound_full = TC.mmd2(f, b, N_REAL, N_FAKE)
    print(f"MARGIN kid seed={seed} shift={shift}: worst error / bound {float((np.abs(values - want_v) / bound_v).max()):.3e}, "
          f"full {abs(full - want_full[0]) / bound_full[0]:.3e}")
    assert (np.abs(values - want_v) <= bound_v).all() and abs(full - want_full[0]) <= bound_full[0]
    out = TS.kid(rd, fd, subsets=subsets, subset_size=size, seed=seed)
    assert set(out) == {"kid_mean", "kid_std", "kid_full", "subsets", "subset_size", "gamma"}
    rounding = (subsets + 4) * TC.U * float(np.abs(want_v).max())
    assert abs(out["kid_mean"] - want_v.mean()) <= bound_v.mean() + rounding
    assert abs(out["kid_std"] - want_v.std()) <= bound_v.max() + rounding        # a standard deviation moves by at most the RMS change
    assert out["kid_full"] == full and (out["subsets"], out["subset_size"]) == (subsets, size)
    assert TS.kid(rd, fd, seed=seed)["subset_size"] == N_FAKE                      # the default: min(n_real, n_fake, 1000)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------
LATENT, N, BATCH, SEEDV, SIZE, E = 100, 12, 5, 11, 64, 40


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    from signature_gan_amd.discriminator_vanilla_gan import Discriminator
    from signature_gan_amd.generator_vanilla_gan import Generator
    torch.manual_seed(7)
    g = Generator(latent_dim=LATENT, output_size=SIZE).to("cuda").eval()
    d = Discriminator(input_size=SIZE).to("cuda").eval()
    with torch.no_grad():
        g.state_dict()["final_conv.0.weight"].mul_(1024.0)
    g._engine.params_changed()
    folder = tmp_path_factory.mktemp("kid_cli")
    ck, vk = folder / "checkpoint.pth", folder / "verifier.pth"
    torch.save({"generator_state_dict": g.state_dict(), "discriminator_state_dict": d.state_dict(),
                "config": {"latent_dim": LATENT, "image_size": SIZE}}, ck)
    torch.save({"model_state_dict": VC.torch_state(E), "embedding_dim": E, "epoch": 1}, vk)
    real = folder / "real"
    real.mkdir()
    from PIL import Image
    rng = np.random.default_rng(5)
    for i in range(9):
        Image.fromarray(rng.integers(0, 256, size=(SIZE, SIZE), dtype=np.uint8), mode="L").save(real / f"r{i}.png")
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


def test_evaluate_verifier_kid(checkpoints, tmp_path, capsys):
    ck, vk, real = checkpoints
    base = ("--real_dir", str(real), "--verifier_checkpoint", str(vk))
    plain = run_evaluate(ck, tmp_path / "p", *base)
    assert "verifier_two_sample" not in plain["metrics"]
    capsys.readouterr()
    flagged = run_evaluate(ck, tmp_path / "k", *base, "--verifier_kid", "99")
    text = capsys.readouterr().out
    block = flagged["metrics"].pop("verifier_two_sample")
    assert scrub(flagged) == scrub(plain)                                  # every other key of the report is what it was
    assert set(block) == {"kid", "mmd_test", "n_real", "n_generated"} and (block["n_real"], block["n_generated"]) == (9, N)
    assert set(block["kid"]) == {"kid_mean", "kid_std", "kid_full", "subsets", "subset_size", "gamma"}
    assert set(block["mmd_test"]) == {"mmd2", "p_value", "null_mean", "null_std", "null_q95", "permutations", "kind", "gamma"}
    assert block["mmd_test"]["permutations"] == 99 and 0 < block["mmd_test"]["p_value"] <= 1
    assert block["mmd_test"]["p_value"] * 100 == pytest.approx(round(block["mmd_test"]["p_value"] * 100))
    assert (block["kid"]["subsets"], block["kid"]["subset_size"], block["kid"]["gamma"]) == (100, 9, 1.0 / E)
    assert all(np.isfinite(v) for v in block["kid"].values()) and all(np.isfinite(v) for k, v in block["mmd_test"].items() if k != "kind")
    assert "Verifier KID: " in text and "Verifier MMD^2 (rbf" in text
    # the default count of permutations, and the flag without a verifier: recorded, the run goes on
    assert run_evaluate(ck, tmp_path / "d", *base, "--verifier_kid")["metrics"]["verifier_two_sample"]["mmd_test"]["permutations"] == 1000
    capsys.readouterr()
    alone = run_evaluate(ck, tmp_path / "n", "--real_dir", str(real), "--verifier_kid", "99")["metrics"]
    assert alone["verifier_two_sample"] is None and "--verifier_checkpoint" in alone["verifier_two_sample_error"]
    assert "Verifier KID: Not computed" in capsys.readouterr().out
    missing = run_evaluate(ck, tmp_path / "m", "--verifier_checkpoint", str(vk), "--verifier_kid", "99")["metrics"]
    assert missing["verifier_two_sample"] is None and missing["verifier_two_sample_error"]
