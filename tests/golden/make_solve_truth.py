"""Writes tests/golden/solve_truth.npz: the solutions of k(Z,Z) V = U for the cases of tests/solve_fixtures.py with M <= 300,
from a Cholesky factorisation and two substitutions in 50-digit arithmetic (mpmath), stored as hi / lo double pairs.  The
matrices and right-hand sides are not stored: the tests regenerate them from the case table and compare their SHA-256 with
the one recorded here.  Offline, a few minutes:  python tests/golden/make_solve_truth.py"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import solve_fixtures as F  # noqa: E402

mp.mp.dps = 50


def solve(k, u):
    """Cholesky (row by row), forward and backward substitution on lists of mpf; k, u: float64 numpy arrays, taken exactly"""
    m, j = u.shape
    a = [[mp.mpf(float(v)) for v in row] for row in k]
    low = [[mp.mpf(0)] * m for _ in range(m)]
    for i in range(m):
        for c in range(i):
            low[i][c] = (a[i][c] - mp.fdot(low[i][:c], low[c][:c])) / low[c][c]
        low[i][i] = mp.sqrt(a[i][i] - mp.fdot(low[i][:i], low[i][:i]))
    upp = [[low[r][c] for r in range(m)] for c in range(m)]  # rows of Lc^T
    hi, lo = np.empty((m, j)), np.empty((m, j))
    for col in range(j):
        y = [mp.mpf(0)] * m
        for i in range(m):
            y[i] = (mp.mpf(float(u[i, col])) - mp.fdot(low[i][:i], y[:i])) / low[i][i]
        x = [mp.mpf(0)] * m
        for i in reversed(range(m)):
            x[i] = (y[i] - mp.fdot(upp[i][i + 1:], x[i + 1:])) / low[i][i]
        for i in range(m):
            hi[i, col] = float(x[i])
            lo[i, col] = float(x[i] - mp.mpf(hi[i, col]))
    return hi, lo


def build(names=None):
    out = {}
    for name in names or F.STORED:
        k, z = F.gram(name)
        u = F.rhs(name, k, z)
        hi, lo = solve(k.numpy(), u.numpy())
        out[f"{name}/hi"], out[f"{name}/lo"] = hi, lo
        out[f"{name}/case"] = np.array(F.CASES[name], dtype=np.float64)  # M, D, seed, lengthscale factor, jitter
        out[f"{name}/sha256"] = np.array(F.checksum(k, u))
        print(name, "done", flush=True)
    return out


if __name__ == "__main__":
    np.savez(F.TRUTH, **build())
