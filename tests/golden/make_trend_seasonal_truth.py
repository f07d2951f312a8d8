"""Writes tests/golden/trend_seasonal_truth.npz for tests/trend_seasonal_truth.py, in 50-digit arithmetic (mpmath), stored as
hi / lo double pairs: per case of CASES the marginal log-likelihood and its gradient (the 4 + 4 d + 1 outputs of pls_gp_mll_grad
for PLS_KERNEL_TREND_SEASONAL), from a Cholesky factorisation, two substitutions, the inverse and the pair sums.  The inputs
are not stored: the tests regenerate them and compare their SHA-256 with the one recorded here.
Offline, a few minutes:  python tests/golden/make_trend_seasonal_truth.py"""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import trend_seasonal_truth as T  # noqa: E402

mp.mp.dps = 50


def coordinate(delta, ls, env, lam, period):
    """(ft, fe, fl, fp) of one coordinate as mpf; sinpi reduces its argument exactly, whatever the size of e"""
    e = delta / period
    return (delta / ls) ** 2, (delta / env) ** 2, 2 / lam * mp.sinpi(e) ** 2, 2 / lam * mp.pi * e * mp.sinpi(2 * e)


def split(values):
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return hi, lo


def evaluate(x, y, diag, ls, env, lam, period, s_t, s_s, mean):
    """one GP with K_y = s_t kappa_t + s_s kappa_s + diag(diag); every float64 input is taken exactly"""
    n, d = x.shape
    s_t, s_s, mean = mp.mpf(float(s_t)), mp.mpf(float(s_s)), mp.mpf(float(mean))
    xm = [[mp.mpf(float(v)) for v in row] for row in x]
    tm, em, lm, pm = ([mp.mpf(float(v)) for v in values] for values in (ls, env, lam, period))
    zero = mp.mpf(0)
    k = [[zero] * n for _ in range(n)]
    # the library's order behind d / d log s_t: d trend lengthscales, d envelope lengthscales, d periodic lengthscales, d period
    # lengths, then d / d log s_s
    dk = [[[zero] * n for _ in range(n)] for _ in range(4 * d + 2)]
    for i in range(n):
        for j in range(i + 1):
            parts = [coordinate(xm[i][c] - xm[j][c], tm[c], em[c], lm[c], pm[c]) for c in range(d)]
            kt = s_t * mp.exp(-mp.fsum(part[0] for part in parts) / 2)
            ks = s_s * mp.exp(-mp.fsum(part[1] / 2 + part[2] for part in parts))
            k[i][j] = k[j][i] = kt + ks
            dk[0][i][j] = dk[0][j][i] = kt
            dk[4 * d + 1][i][j] = dk[4 * d + 1][j][i] = ks
            for c in range(d):
                dk[1 + c][i][j] = dk[1 + c][j][i] = kt * parts[c][0]
                for block in range(1, 4):
                    dk[1 + block * d + c][i][j] = dk[1 + block * d + c][j][i] = ks * parts[c][block]
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
    out = [zero] * (4 + 4 * d + 1)
    out[0] = -mp.fdot(r, alpha) / 2 - mp.fsum(mp.log(low[i][i]) for i in range(n)) - mp.mpf(n) / 2 * mp.log(2 * mp.pi)
    out[1] = mp.fsum(alpha)
    out[2] = mp.fsum(alpha[i] * alpha[i] - p[i][i] for i in range(n)) / 2
    w = [[alpha[i] * alpha[j] - p[i][j] for j in range(n)] for i in range(n)]
    for c in range(4 * d + 2):
        out[3 + c] = mp.fsum(mp.fdot(w[i], dk[c][i]) for i in range(n)) / 2
    return split(out)


def one(name):
    x, y, ls, env, lam, period = T.case_inputs(name)
    hi, lo = evaluate(x.numpy(), y.numpy(), [T.NOISE] * x.shape[0], ls.numpy(), env.numpy(), lam.numpy(), period.numpy(), T.S_T,
                      T.S_S, T.MEAN)
    print(name, "done", flush=True)
    return name, hi, lo, T.checksum([x, y, ls, env, lam, period])


def build(processes=None):
    out = {}
    with multiprocessing.Pool(processes) as pool:
        for name, hi, lo, sha in pool.imap_unordered(one, sorted(T.CASES, key=lambda k: -T.CASES[k][0])):
            out[f"{name}/hi"], out[f"{name}/lo"] = hi, lo
            out[f"{name}/case"] = np.array(T.CASES[name], dtype=np.float64)  # n, d, seed
            out[f"{name}/sha256"] = np.array(sha)
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
