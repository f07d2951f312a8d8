"""Inputs and truth of the symmetric eigensolver tests (tests/test_sym_eigh_host.py, tests/test_gpu_sym_eigh.py).

Four families of symmetric matrices, seeded per (family, M):
  rbf       RBF Gram / M of d = 2 standard-normal points, lengthscale 0.6: rank-deficient to rounding
  matern12  Matern-1/2 Gram / M of such points: well separated eigenvalues
  indef     K / M - 6 K K^T / M^2 with K an RBF Gram matrix: indefinite, as the predictive covariance is
  doubled   diag(B, B) with B = matern12 of order M // 2 (an odd M gets one more 1 x 1 block, B[0, 0]): every eigenvalue of
            the two big blocks is double, so eigenvectors are not unique
tests/golden/sym_eigh_truth.npz (made by tests/golden/make_sym_eigh_truth.py) holds, for M in FIXTURE_SIZES, the lower
triangle of each matrix -- the bits the truth belongs to -- and its eigenvalues from mpmath.eigsy at 50 digits."""
import os

import numpy as np

FAMILIES = ("rbf", "matern12", "indef", "doubled")
FIXTURE_SIZES = (3, 17, 64, 65, 96, 130)
EPS = float(np.finfo(np.float64).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sym_eigh_truth.npz")


def _points(m, seed):
    return np.random.default_rng([seed, m]).standard_normal((m, 2))


def _sqdist(x):
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def make_matrix(family, m):
    """The (m, m) float64 matrix of `family`, generated (not read from the fixture)."""
    if family == "rbf":
        return np.exp(-_sqdist(_points(m, 1)) / (2 * 0.6**2)) / m
    if family == "matern12":
        return np.exp(-np.sqrt(_sqdist(_points(m, 2))) / 0.6) / m
    if family == "indef":
        k = np.exp(-_sqdist(_points(m, 3)) / (2 * 0.6**2))
        a = k / m - 6.0 * (k @ k.T) / m**2
        return (a + a.T) / 2
    if family == "doubled":
        h = m // 2
        a = np.zeros((m, m))
        if h:
            b = make_matrix("matern12", h)
            a[:h, :h] = b
            a[h:2 * h, h:2 * h] = b
        if m % 2:
            a[m - 1, m - 1] = a[0, 0] if h else 1.0
        return a
    raise ValueError(family)


_truth = None


def load_truth():
    """{(family, m): (matrix, eigenvalues ascending)} of the committed fixture."""
    global _truth
    if _truth is None:
        z = np.load(GOLDEN)
        out = {}
        for family in FAMILIES:
            for m in FIXTURE_SIZES:
                tri = z[f"{family}_{m}_tril"]
                a = np.zeros((m, m))
                a[np.tril_indices(m)] = tri
                a = a + np.tril(a, -1).T
                out[(family, m)] = (a, z[f"{family}_{m}_lam"])
        _truth = out
    return _truth


def case(family, m):
    """(matrix, reference eigenvalues, where the reference comes from) -- the fixture where it has the case, else LAPACK."""
    if m in FIXTURE_SIZES:
        a, lam = load_truth()[(family, m)]
        return a.copy(), lam.copy(), "mpmath"
    a = make_matrix(family, m)
    return a, np.linalg.eigvalsh(a), "lapack"
