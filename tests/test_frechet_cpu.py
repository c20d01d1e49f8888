"""The host side of the verifier Frechet distance (utils/frechet.py, the evaluation CLI's flag and report keys): the
moments -> (mean, cov) arithmetic against np.cov, the distance against closed forms and against the definition written
out, and the CLI's opt-in behaviour.  Nothing here needs a GPU; tests/test_moments_gpu.py checks the accumulator kernel."""
import io
import json
from contextlib import redirect_stdout

import numpy as np
import pytest
import scipy.linalg

import signature_gan_amd  # noqa: F401  (import shim for signature-gan_amd/)
from signature_gan_amd.utils.frechet import embedding_spread, frechet_distance, stats_from_moments

U = 2.0 ** -53


def grid_rows(n, d, seed):
    """Random fp32 rows with |x| <= 1 on the 2^-12 grid whose column means lie on the grid too.  Sums of at most 300 such
    values or products need 34 bits, so s, G AND the centred sums inside np.cov are exact in fp64 whatever order a BLAS adds
    them in: the comparison below measures stats_from_moments alone.  (With uniform values np.cov's own 300-term sums sit
    0.5 to 1.3 of the bound away from an 80-bit covariance, the helper 0.05.)"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-2048, 2049, (n, d))
    total = v.sum(axis=0)
    v -= total // n                                                         # column sums into 0..n-1 ...
    for j, rest in enumerate(total % n):
        v[:rest, j] -= 1                                                    # ... and to zero
    assert not v.sum(axis=0).any()
    v += rng.integers(-1024, 1025, d)                                       # column means k / 4096, mostly non-zero
    x = (v / 4096.0).astype(np.float32)
    assert np.abs(x).max() <= 1 and np.array_equal(x.astype(np.float64) * 4096, v)
    return x


@pytest.mark.parametrize("n", [7, 300])
def test_stats_from_moments_is_np_cov(n):
    """s and G formed by numpy in fp64 from fp32 rows with |x| <= 1, D = 40.  Every term of G - n mu mu^T is at most n in
    magnitude and a handful of roundings apart on either side: 8 n 2^-53 / (n - 1) absolute per entry."""
    d = 40
    x = grid_rows(n, d, n).astype(np.float64)
    got_n, mean, cov = stats_from_moments(n, x.sum(axis=0), x.T @ x)
    bound = 8 * n * U / (n - 1)
    e_cov = float(np.abs(cov - np.cov(x, rowvar=False)).max())
    e_mean = float(np.abs(mean - x.mean(axis=0)).max())
    print(f"n={n}: cov error {e_cov:.3e}, mean error {e_mean:.3e}, bound {bound:.3e}")
    assert got_n == n and mean.dtype == np.float64 and cov.dtype == np.float64 and cov.shape == (d, d)
    assert np.abs(mean).max() > 0.1                                         # the n mu mu^T term is there to be got wrong
    assert e_cov <= bound and e_mean <= bound
    assert np.array_equal(cov, cov.T)                                       # symmetrised
    assert abs(embedding_spread(cov) - np.trace(np.cov(x, rowvar=False))) <= d * bound


@pytest.mark.parametrize("n", [1, 0, -3])
def test_fewer_than_two_rows_raise(n):
    """The helper FeatureMoments.finish ends in, called directly: no device needed."""
    with pytest.raises(ValueError, match="at least 2"):
        stats_from_moments(n, np.zeros(4), np.zeros((4, 4)))


def _spd(rng, d, n):
    a = rng.standard_normal((d, n))
    return a @ a.T / n + 0.1 * np.eye(d)


def test_frechet_distance_closed_forms():
    """Diagonal covariances, D = 128, entries in [0.1, 2]: ||dmu||^2 + sum (sqrt a - sqrt b)^2.  Both sides are O(D) fp64
    roundings (about 1e-14 relative), 1e-9 leaves five orders.  The distance of a set to itself is 0 to 1e-9 tr(sigma), and
    the function is symmetric in its two sets to the same bound."""
    rng = np.random.default_rng(11)
    d = 128
    a, b = rng.uniform(0.1, 2.0, d), rng.uniform(0.1, 2.0, d)
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    want = float(((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum())
    got = frechet_distance(mu1, np.diag(a), mu2, np.diag(b))
    print(f"diagonal: got {got!r} want {want!r} rel {abs(got - want) / want:.3e}")
    assert isinstance(got, float) and abs(got - want) <= 1e-9 * want

    s1, s2 = _spd(rng, d, 4 * d), _spd(rng, d, 4 * d)
    tol = 1e-9 * float(np.trace(s1))
    same = frechet_distance(mu1, s1, mu1, s1)
    fwd, bwd = frechet_distance(mu1, s1, mu2, s2), frechet_distance(mu2, s2, mu1, s1)
    print(f"self distance {same:.3e}, asymmetry {abs(fwd - bwd):.3e}, tolerance {tol:.3e}")
    assert abs(same) <= tol
    assert abs(fwd - bwd) <= tol and fwd > 0
    assert embedding_spread(s1) == float(np.trace(s1))


def test_frechet_distance_is_the_definition():
    """A general SPD pair (sigma = A A^T / n + 0.1 I, D = 40) against the definition written out: the same arithmetic."""
    rng = np.random.default_rng(12)
    d = 40
    s1, s2 = _spd(rng, d, 60), _spd(rng, d, 45)
    mu1, mu2 = rng.standard_normal(d), rng.standard_normal(d)
    root = scipy.linalg.sqrtm(s1 @ s2)
    if np.iscomplexobj(root):
        root = root.real
    diff = mu1 - mu2
    want = float(diff @ diff + np.trace(s1 + s2 - 2 * root))
    got = frechet_distance(mu1, s1, mu2, s2)
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert got == frechet_distance(mu1.astype(np.float64).tolist(), s1, mu2, s2)      # anything array-like
    with pytest.raises(ValueError):
        frechet_distance(mu1, s1, mu2[:-1], s2)


def test_cli_flag_is_opt_in():
    from signature_gan_amd.evaluate_vanilla_gan_signatures import parse_args
    a = parse_args(["--checkpoint", "ck.pt"])
    assert a.verifier_checkpoint is None
    assert "verifier_checkpoint" not in vars(a)            # a command line without the flag parses as it always did
    b = parse_args(["--checkpoint", "ck.pt", "--verifier_checkpoint", "v.pth", "--real_dir", "r"])
    assert b.verifier_checkpoint == "v.pth" and vars(b)["verifier_checkpoint"] == "v.pth" and b.real_dir == "r"


def test_report_summary_and_printed_line(tmp_path):
    """A report made without the flag keeps its summary keys and its stdout; the distance joins both when the metrics
    dictionary has the key -- as a number, or as None with the recorded reason."""
    from signature_gan_amd.evaluate_vanilla_gan_signatures import print_summary, save_evaluation_report
    five = {"fid_score", "lpips_diversity", "stroke_density_mean", "foreground_ratio_mean", "n_samples_evaluated"}
    stroke = {"mean": 0.25, "std": 0.1, "min": 0.0, "max": 0.5}
    base = {"n_samples": 4, "image_shape": [1, 64, 64], "fid_score": None, "fid_error": "x", "lpips_diversity": None,
            "lpips_error": "y", "stroke_density": stroke, "foreground_ratio": {"mean": 0.25, "std": 0.1}}

    def run(metrics):
        out = io.StringIO()
        with redirect_stdout(out):
            path = save_evaluation_report(metrics, {}, tmp_path, tmp_path / "ck.pt", [])
            print_summary(metrics)
        with open(path) as f:
            return json.load(f)["summary"], out.getvalue()

    summary, text = run(dict(base))
    assert set(summary) == five and "Verifier" not in text
    assert summary == {"fid_score": None, "lpips_diversity": None, "stroke_density_mean": 0.25, "foreground_ratio_mean": 0.25,
                       "n_samples_evaluated": 4}
    summary, text = run(dict(base, verifier_frechet_distance=None, verifier_frechet_error="no real images provided"))
    assert set(summary) == five | {"verifier_frechet_distance"} and summary["verifier_frechet_distance"] is None
    assert "Verifier Frechet Distance: Not computed - no real images provided" in text
    summary, text = run(dict(base, verifier_frechet_distance=0.125))
    assert summary["verifier_frechet_distance"] == 0.125
    lines = text.splitlines()
    at = lines.index("Verifier Frechet Distance: 0.1250 (lower is better)")
    assert lines.index("--- Quality Metrics ---") < at < lines.index("--- Stroke Analysis ---")


def test_library_exports_the_moments_header():
    import ctypes as C
    import os
    import re
    from common import ROOT
    from signature_gan_amd import _lib
    with open(os.path.join(ROOT, "include", "siggan_moments.h")) as f:
        declared = set(re.findall(r"\bint\s+(siggan_\w+)\s*\(", f.read()))
    assert declared == set(_lib.MOMENTS_EXPORTS) and len(declared) == 5
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in siggan_moments.h but not exported"
    assert lib.siggan_abi_version() == 4                   # symbols only added
    h = C.c_void_p()
    for dim in (0, _lib.MOMENTS_MAX_DIM + 1, -5):          # refused before anything touches a device
        assert lib.siggan_moments_create(0, dim, C.byref(h)) == _lib.E_ARG and not h.value
        assert b"dim" in lib.siggan_last_error()
