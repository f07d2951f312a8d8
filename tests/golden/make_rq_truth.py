"""Writes tests/golden/rq_truth.npz for tests/rq_truth.py, in 50-digit arithmetic (mpmath), stored as hi / lo double pairs:
"pairs": kappa, g = kappa / (1 + u) and ga = alpha kappa (u / (1 + u) - log1p(u)) of the rational-quadratic kernel per
alpha and squared distance of the table PAIR_R2; per case of CASES the marginal log-likelihood and its gradient (the 5 + d
outputs of pls_gp_mll_grad for PLS_KERNEL_RQ), from a Cholesky factorisation, two substitutions, the inverse and the pair
sums.  The inputs are not stored: the tests regenerate them and compare their SHA-256 with the one recorded here.
Offline, a minute or two:  python tests/golden/make_rq_truth.py"""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import rq_truth as T  # noqa: E402

mp.mp.dps = 50


def pair(r2, shape):
    """(kappa, g, ga) of one pair as mpf"""
    u = r2 / (2 * shape)
    kap = mp.exp(-shape * mp.log1p(u))
    return kap, kap / (1 + u), shape * kap * (u / (1 + u) - mp.log1p(u))


def split(values):
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return hi, lo


def pairs_table():
    # (700 digits here: at r^2 = 1e-300 the two terms of ga agree in their first 300 digits)
    with mp.workdps(700):
        return _pairs_table()


def _pairs_table():
    flat = [f for a in T.ALPHAS for f in zip(*[pair(mp.mpf(float(r2)), mp.mpf(float(a))) for r2 in T.PAIR_R2])]
    hi, lo = split([v for row in flat for v in row])
    shape = (len(T.ALPHAS), 3, len(T.PAIR_R2))
    return hi.reshape(shape), lo.reshape(shape)


def evaluate(x, y, diag, ls, shape, s, mean):
    """one GP with K_y = s kappa + diag(diag); every float64 input is taken exactly"""
    n, d = x.shape
    s, mean, shape = mp.mpf(float(s)), mp.mpf(float(mean)), mp.mpf(float(shape))
    xm = [[mp.mpf(float(v)) for v in row] for row in x]
    lm = [mp.mpf(float(v)) for v in ls]
    zero = mp.mpf(0)
    k = [[zero] * n for _ in range(n)]
    dk = [[[zero] * n for _ in range(n)] for _ in range(d + 1)]  # d lengthscales, then alpha
    for i in range(n):
        for j in range(i + 1):
            e2 = [((xm[i][c] - xm[j][c]) / lm[c]) ** 2 for c in range(d)]
            kap, g, ga = pair(mp.fsum(e2), shape)
            k[i][j] = k[j][i] = s * kap
            for c in range(d):
                dk[c][i][j] = dk[c][j][i] = s * g * e2[c]
            dk[d][i][j] = dk[d][j][i] = s * ga
    a = [[k[i][j] + (mp.mpf(float(diag[i])) if i == j else 0) for j in range(n)] for i in range(n)]
    low = [[zero] * n for _ in range(n)]
    for i in range(n):
        for c in range(i):
            low[i][c] = (a[i][c] - mp.fdot(low[i][:c], low[c][:c])) / low[c][c]
        low[i][i] = mp.sqrt(a[i][i] - mp.fdot(low[i][:i], low[i][:i]))
    cols = [[zero] * n for _ in range(n)]  # cols[c][i] = (Lc^-1)[i][c]
    for c in range(n):
        col = cols[c]
        for i in range(c, n):
            col[i] = ((1 if i == c else 0) - mp.fdot(low[i][c:i], col[c:i])) / low[i][i]
    p = [[zero] * n for _ in range(n)]  # K_y^-1
    for i in range(n):
        for j in range(i + 1):
            p[i][j] = p[j][i] = mp.fdot(cols[i][i:], cols[j][i:])
    r = [mp.mpf(float(v)) - mean for v in y]
    alpha = [mp.fdot(p[i], r) for i in range(n)]
    out = [zero] * (5 + d)
    out[0] = -mp.fdot(r, alpha) / 2 - mp.fsum(mp.log(low[i][i]) for i in range(n)) - mp.mpf(n) / 2 * mp.log(2 * mp.pi)
    out[1] = mp.fsum(alpha)
    out[2] = mp.fsum(alpha[i] * alpha[i] - p[i][i] for i in range(n)) / 2
    w = [[alpha[i] * alpha[j] - p[i][j] for j in range(n)] for i in range(n)]
    out[3] = mp.fsum(mp.fdot(w[i], k[i]) for i in range(n)) / 2
    for c in range(d + 1):
        out[4 + c] = mp.fsum(mp.fdot(w[i], dk[c][i]) for i in range(n)) / 2
    return split(out)


def one(name):
    x, y, ls, shape = T.case_inputs(name)
    hi, lo = evaluate(x.numpy(), y.numpy(), [T.NOISE] * x.shape[0], ls.numpy(), shape, T.OUTPUTSCALE, T.MEAN)
    print(name, "done", flush=True)
    return name, hi, lo, T.checksum([x, y, ls])


def build(processes=None):
    out = {}
    out["pairs/hi"], out["pairs/lo"] = pairs_table()
    out["pairs/sha256"] = np.array(T.checksum([torch.from_numpy(T.PAIR_R2), torch.tensor(T.ALPHAS, dtype=torch.float64)]))
    with multiprocessing.Pool(processes) as pool:
        for name, hi, lo, sha in pool.imap_unordered(one, sorted(T.CASES, key=lambda k: -T.CASES[k][0])):
            out[f"{name}/hi"], out[f"{name}/lo"] = hi, lo
            out[f"{name}/case"] = np.array(T.CASES[name], dtype=np.float64)  # n, d, seed, alpha
            out[f"{name}/sha256"] = np.array(sha)
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
