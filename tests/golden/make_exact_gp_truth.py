"""Writes tests/golden/exact_gp_truth.npz: the exact-GP marginal log-likelihood and its gradient (the 4 + d outputs of
pls_gp_mll_grad) for the cases of tests/exact_gp_truth.py, from a Cholesky factorisation, two substitutions, the inverse
and the pair sums in 50-digit arithmetic (mpmath), stored as hi / lo double pairs.  The inputs are not stored: the tests
regenerate them from the case table and compare their SHA-256 with the one recorded here.  Offline, a few minutes on a
few cores:  python tests/golden/make_exact_gp_truth.py"""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import exact_gp_truth as T  # noqa: E402

mp.mp.dps = 50


def kernel_and_derivatives(kind, x, ls, s):
    """K (without noise) and dK / d log l_k for i >= j as lists of mpf; x, ls float64 numpy arrays, taken exactly"""
    n, d = x.shape
    xm = [[mp.mpf(float(v)) for v in row] for row in x]
    lm = [mp.mpf(float(v)) for v in ls]
    zero = mp.mpf(0)
    k = [[zero] * n for _ in range(n)]
    dk = [[[zero] * n for _ in range(n)] for _ in range(d)]
    for i in range(n):
        for j in range(i + 1):
            e2 = [((xm[i][c] - xm[j][c]) / lm[c]) ** 2 for c in range(d)]
            r2 = mp.fsum(e2)
            if kind == T.RBF:
                ex = mp.exp(-r2 / 2)
                kap, g = ex, ex
            else:
                nu = mp.mpf(T.NU[kind])
                t = mp.sqrt(2 * nu * r2)
                ex = mp.exp(-t)
                kap = ex * (1 if kind == T.MATERN12 else 1 + t if kind == T.MATERN32 else 1 + t + t * t / 3)
                q = (1 / t if t > 0 else zero) if kind == T.MATERN12 else (mp.mpf(1) if kind == T.MATERN32 else (1 + t) / 3)
                g = q * ex * 2 * nu
            k[i][j] = k[j][i] = s * kap
            for c in range(d):
                dk[c][i][j] = dk[c][j][i] = s * g * e2[c]
    return k, dk


def evaluate(kind, x, y, diag, ls, s, mean):
    """one GP with K_y = s kappa + diag(diag); every float64 input is taken exactly"""
    n, d = x.shape
    s, mean = mp.mpf(float(s)), mp.mpf(float(mean))
    k, dk = kernel_and_derivatives(kind, x, ls, s)
    a = [[k[i][j] + (mp.mpf(float(diag[i])) if i == j else 0) for j in range(n)] for i in range(n)]
    low = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for c in range(i):
            low[i][c] = (a[i][c] - mp.fdot(low[i][:c], low[c][:c])) / low[c][c]
        low[i][i] = mp.sqrt(a[i][i] - mp.fdot(low[i][:i], low[i][:i]))
    # rows of Linv = Lc^-1 (lower): Linv[i][c] = (delta_ic - sum_{c <= m < i} Lc[i][m] Linv[m][c]) / Lc[i][i]
    cols = [[mp.mpf(0)] * n for _ in range(n)]  # cols[c][i] = Linv[i][c]
    for c in range(n):
        col = cols[c]
        for i in range(c, n):
            col[i] = ((1 if i == c else 0) - mp.fdot(low[i][c:i], col[c:i])) / low[i][i]
    # P = K_y^-1 = Linv^T Linv:  P[i][j] = sum_{m >= max(i, j)} Linv[m][i] Linv[m][j]
    p = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            p[i][j] = p[j][i] = mp.fdot(cols[i][i:], cols[j][i:])
    r = [mp.mpf(float(v)) - mean for v in y]
    alpha = [mp.fdot(p[i], r) for i in range(n)]
    out = [mp.mpf(0)] * (4 + d)
    out[0] = -mp.fdot(r, alpha) / 2 - mp.fsum(mp.log(low[i][i]) for i in range(n)) - mp.mpf(n) / 2 * mp.log(2 * mp.pi)
    out[1] = mp.fsum(alpha)
    out[2] = mp.fsum(alpha[i] * alpha[i] - p[i][i] for i in range(n)) / 2
    w = [[alpha[i] * alpha[j] - p[i][j] for j in range(n)] for i in range(n)]
    out[3] = mp.fsum(mp.fdot(w[i], k[i]) for i in range(n)) / 2  # d / d log s: dK / d log s = K (without the noise)
    for c in range(d):
        out[4 + c] = mp.fsum(mp.fdot(w[i], dk[c][i]) for i in range(n)) / 2
    hi = np.array([float(v) for v in out])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(out, hi)])
    return hi, lo


def one(name):
    kind, x, y, ls = T.case_inputs(name)
    hi, lo = evaluate(kind, x.numpy(), y.numpy(), [T.NOISE] * x.shape[0], ls.numpy(), T.OUTPUTSCALE, T.MEAN)
    print(name, "done", flush=True)
    return name, hi, lo, T.checksum([x, y, ls])


def build(names=None, processes=None):
    names = sorted(names or T.CASES, key=lambda k: -T.CASES[k][1])  # the largest first
    out = {}
    with multiprocessing.Pool(processes) as pool:
        for name, hi, lo, sha in pool.imap_unordered(one, names):
            out[f"{name}/hi"], out[f"{name}/lo"] = hi, lo
            out[f"{name}/case"] = np.array(T.CASES[name], dtype=np.float64)  # kind, n, d, seed
            out[f"{name}/sha256"] = np.array(sha)
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
