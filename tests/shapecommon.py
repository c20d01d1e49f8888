"""Shared by the shape-attribute tests: seeded numpy builders of their images (fp32 in [-1, 1], +1 paper, -1 ink) and of the
weights and targets of an objective.  The REGULAR inputs -- the random smooth images and the slanted bar -- are built to have
mass >= 0.02 and syy >= 1e-3 (asserted here): the tolerances of the tests are worked out for those."""
import numpy as np

SIZES = (64, 128)
MIN_MASS, MIN_SYY = 0.02, 1e-3


def smooth_images(n, s, seed):
    """(n, s, s) fp32: a coarse random field blown up and blurred, with a little per-pixel noise so that no value is round."""
    rng = np.random.default_rng(seed)
    field = np.kron(rng.normal(size=(n, s // 8, s // 8)), np.ones((8, 8)))
    for shift in (1, 2, 3):
        field = (field + np.roll(field, shift, axis=1) + np.roll(field, shift, axis=2)) / 3.0
    ink = np.clip(0.35 + 0.9 * field + rng.normal(0.0, 0.02, size=field.shape), 0.0, 1.0)
    return (1.0 - 2.0 * ink).astype(np.float32)


def slanted_bar(s, k=-0.5, half_width=0.06, half_height=0.3):
    """(s, s) fp32: full ink where |u - k v| < half_width and |v| < half_height.  k < 0 leans to the right ("/")."""
    t = (np.arange(s) + 0.5) / s - 0.5
    v, u = np.meshgrid(t, t, indexing="ij")
    return np.where((np.abs(u - k * v) < half_width) & (np.abs(v) < half_height), -1.0, 1.0).astype(np.float32)


def regular_images(n, s, seed=0):
    """(n, s, s) fp32: n - 1 smooth images and the slanted bar (last), with the guarantees of the module docstring."""
    from signature_gan_amd.shape import MASS, SYY, reference_features
    x = np.concatenate([smooth_images(n - 1, s, seed + s), slanted_bar(s)[None]]) if n > 1 else slanted_bar(s)[None]
    f = reference_features(x)
    assert (f[:, MASS] >= MIN_MASS).all() and (f[:, SYY] >= MIN_SYY).all(), (f[:, MASS].min(), f[:, SYY].min())
    return x


def blank(s):
    return np.ones((s, s), dtype=np.float32)


def corner_pixel(s):
    x = blank(s)
    x[0, 0] = -1.0
    return x


def ink_row(s, row=None):
    """One horizontal row of full ink: syy is exactly 0."""
    x = blank(s)
    x[s // 3 if row is None else row, :] = -1.0
    return x


def all_ink(s):
    return -np.ones((s, s), dtype=np.float32)


def objective_rows(n, features, seed=1):
    """(weights, targets) fp64 (n, 8): every weight in [0.5, 2], every target the feature moved by a tenth of its size (at
    least 0.01), so that every term contributes to the gradient."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, size=(n, 8))
    t = features + rng.choice([-1.0, 1.0], size=(n, 8)) * np.maximum(0.1 * np.abs(features), 0.01)
    return w, t
