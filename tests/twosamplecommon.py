"""The numpy fp64 restatement of siggan_kernel_forms (include/siggan_twosample.h) and the error bounds the GPU tests hold it
to.  K from direct sums, d2 as sum_k (a_k - b_k)^2; the diagonal zeroed by position; the forms as (A * (K0 @ A)).sum(0).

Bounds, derived and not tuned, with U = 2^-52 (twice the unit roundoff: one for the device, one for this file, the convention
of test_neighbors_gpu.py).  Every product of two widened fp32 values is exact in fp64.

* poly, k = t^d with t = gamma a.b + coef0.  The dot product is a sum of dim exact products in some order: within
  dim u |a||b| of the truth.  gamma * dot and + coef0 round once each, so with T = gamma |a||b| + |coef0| >= |t|:
  |dt| <= (dim + 2) u T.  The power by d - 1 multiplications: |dk| <= d T^(d-1) |dt| + (d - 1) u T^d
  <= (d (dim + 2) + d) u T^d.  Both sides: Bk_ij = d (dim + 3) U T_ij^d.
* rbf, k = exp(-gamma d2).  d2 as in test_neighbors_gpu.py: B_ij = (dim + 4) U (|a| + |b|)^2 covers both sides.  The
  argument gamma * d2 rounds once per side, exp is within 1 ulp <= U of the true exponential on either side (the device
  library's stated fp64 exp error; the host's is below that), and exp turns an absolute error of its argument into a relative
  one of its value: Bk_ij = k_ij (gamma B_ij + |arg| U + 2 U).  (First order: the second-order terms are 1e-13 times smaller.)
* a form is a sum of `terms` such values (adding an exact 0 costs nothing): in any order within terms u sum |k| per side, so
  B_form = sum Bk_ij + terms U sum |k_ij| over the pairs the form holds.
* MMD^2_u = F_AA / (na (na - 1)) + F_BB / (nb (nb - 1)) - 2 F_AB / (na nb): the three form bounds divided alike, plus four
  roundings of the quotients and sums on either side: 4 U times the sum of the three terms' magnitudes."""
import numpy as np

U = 2.0 ** -52


def kernel_matrix(x, kind, gamma, coef0=1.0, degree=3):
    """(K (n, n), Bk (n, n)) in fp64 from the fp32 rows x; the diagonal is still there."""
    x64 = x.astype(np.float64)
    dim = x.shape[1]
    norm = np.sqrt((x64 ** 2).sum(axis=1))
    if kind == "poly":
        dot = (x64[:, None, :] * x64[None, :, :]).sum(axis=2)
        t = gamma * dot + coef0
        k = t if degree == 1 else t * t if degree == 2 else (t * t) * t
        big = gamma * norm[:, None] * norm[None, :] + abs(coef0)
        return k, degree * (dim + 3) * U * big ** degree
    d2 = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2)
    arg = gamma * d2
    k = np.exp(-arg)
    b_d2 = (dim + 4) * U * (norm[:, None] + norm[None, :]) ** 2
    return k, k * (gamma * b_d2 + arg * U + 2 * U)


def forms(x, labels, kind, gamma, coef0=1.0, degree=3):
    """(forms (cols, 3), bound (cols, 3), diag (n)): the restatement and B_form per entry."""
    k, bk = kernel_matrix(x, kind, gamma, coef0, degree)
    diag = np.diagonal(k).copy()
    k0, bk0 = k.copy(), bk.copy()
    np.fill_diagonal(k0, 0.0)
    np.fill_diagonal(bk0, 0.0)
    a, b = (labels == 1).astype(np.float64), (labels == 2).astype(np.float64)
    na, nb = a.sum(axis=0), b.sum(axis=0)
    out = np.stack([(a * (k0 @ a)).sum(0), (b * (k0 @ b)).sum(0), (a * (k0 @ b)).sum(0)], axis=1)
    ak0 = np.abs(k0)
    mag = np.stack([(a * (ak0 @ a)).sum(0), (b * (ak0 @ b)).sum(0), (a * (ak0 @ b)).sum(0)], axis=1)
    err = np.stack([(a * (bk0 @ a)).sum(0), (b * (bk0 @ b)).sum(0), (a * (bk0 @ b)).sum(0)], axis=1)
    terms = np.stack([na * (na - 1), nb * (nb - 1), na * nb], axis=1)
    return out, err + terms * U * mag, diag


def mmd2(f, bound, na, nb):
    """(MMD^2_u (cols), its bound (cols)) from forms (cols, 3) and their bounds."""
    f, bound = np.asarray(f, np.float64).reshape(-1, 3), np.asarray(bound, np.float64).reshape(-1, 3)
    w = np.array([1.0 / (na * (na - 1)), 1.0 / (nb * (nb - 1)), 2.0 / (na * nb)])
    value = f[:, 0] * w[0] + f[:, 1] * w[1] - f[:, 2] * w[2]
    return value, (bound * w).sum(axis=1) + 4 * U * (np.abs(f) * w).sum(axis=1)


def median_gamma(rows):
    r = rows.astype(np.float64)
    d2 = ((r[:, None, :] - r[None, :, :]) ** 2).sum(axis=2)
    return 1.0 / float(np.median(d2[np.triu_indices(len(r), 1)]))


def integer_rows(n, dim, seed=0):
    """fp32 rows with entries in {-2, .., 2}: every kernel value and every sum of them is an integer far below 2^53."""
    return np.random.default_rng([seed, n, dim]).integers(-2, 3, size=(n, dim)).astype(np.float32)


def random_labels(n, cols, seed=0):
    """uint8 (n, cols) over {0, 1, 2}, the three about equally often."""
    return np.random.default_rng([seed, n, cols, 7]).integers(0, 3, size=(n, cols)).astype(np.uint8)


def float_rows(family, n, dim, seed=0):
    """'normal': standard-normal rows; 'unit': unit-norm rows of which every fifth is a near copy (1e-4 noise) of another --
    the cancellation case of test_neighbors_gpu.py."""
    rng = np.random.default_rng([seed, n, dim, 0 if family == "normal" else 1])
    x = rng.standard_normal((n, dim))
    if family == "unit":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        for j in range(0, n, 5):
            x[j] = x[(j + 1) % n] + 1e-4 * rng.standard_normal(dim)
    return x.astype(np.float32)
