"""Writes tests/golden/locally_periodic_truth.npz for tests/locally_periodic_truth.py, in 50-digit arithmetic (mpmath), stored as
hi / lo double pairs: "pairs": kappa, fe = (delta / l)^2, fl = (2 / lambda) sin^2(pi e) and fp = (2 / lambda) pi e sin(2 pi e)
of the locally periodic kernel per period length and difference of the table pair_deltas() (e = delta / p taken exactly from
the float64 delta and p); per case of CASES the marginal log-likelihood and its gradient (the 4 + 3 d outputs of
pls_gp_mll_grad for PLS_KERNEL_LOCALLY_PERIODIC), from a Cholesky factorisation, two substitutions, the inverse and the pair
sums.  The inputs are not stored: the tests regenerate them and compare their SHA-256 with the one recorded here.
Offline, a few minutes:  python tests/golden/make_locally_periodic_truth.py"""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import locally_periodic_truth as T  # noqa: E402

mp.mp.dps = 50


def coordinate(delta, ls, lam, period):
    """(fe, fl, fp) of one coordinate as mpf; sinpi reduces its argument exactly, whatever the size of e"""
    e = delta / period
    return (delta / ls) ** 2, 2 / lam * mp.sinpi(e) ** 2, 2 / lam * mp.pi * e * mp.sinpi(2 * e)


def pair_kappa(parts):
    return mp.exp(-mp.fsum(fe / 2 + fl for fe, fl, _ in parts))


def split(values):
    hi = np.array([float(v) for v in values])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(values, hi)])
    return hi, lo


def pairs_table():
    lam, ls = mp.mpf(float(T.PAIR_PERIODIC_LENGTHSCALE)), mp.mpf(float(T.PAIR_LENGTHSCALE))
    flat = []
    for p, row in zip(T.PAIR_PERIODS, T.pair_deltas()):
        parts = [coordinate(mp.mpf(float(delta)), ls, lam, mp.mpf(float(p))) for delta in row]
        flat += [[pair_kappa([part]) for part in parts]] + [[part[c] for part in parts] for c in range(3)]
    hi, lo = split([v for row in flat for v in row])
    shape = (len(T.PAIR_PERIODS), 4, len(T.PAIR_E))
    return hi.reshape(shape), lo.reshape(shape)


def evaluate(x, y, diag, ls, lam, period, s, mean):
    """one GP with K_y = s kappa + diag(diag); every float64 input is taken exactly"""
    n, d = x.shape
    s, mean = mp.mpf(float(s)), mp.mpf(float(mean))
    xm = [[mp.mpf(float(v)) for v in row] for row in x]
    em, lm, pm = ([mp.mpf(float(v)) for v in values] for values in (ls, lam, period))
    zero = mp.mpf(0)
    k = [[zero] * n for _ in range(n)]
    dk = [[[zero] * n for _ in range(n)] for _ in range(3 * d)]  # d envelope lengthscales, d periodic lengthscales, d period lengths
    for i in range(n):
        for j in range(i + 1):
            parts = [coordinate(xm[i][c] - xm[j][c], em[c], lm[c], pm[c]) for c in range(d)]
            kap = pair_kappa(parts)
            k[i][j] = k[j][i] = s * kap
            for c in range(d):
                for block in range(3):
                    dk[block * d + c][i][j] = dk[block * d + c][j][i] = s * kap * parts[c][block]
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
    out = [zero] * (4 + 3 * d)
    out[0] = -mp.fdot(r, alpha) / 2 - mp.fsum(mp.log(low[i][i]) for i in range(n)) - mp.mpf(n) / 2 * mp.log(2 * mp.pi)
    out[1] = mp.fsum(alpha)
    out[2] = mp.fsum(alpha[i] * alpha[i] - p[i][i] for i in range(n)) / 2
    w = [[alpha[i] * alpha[j] - p[i][j] for j in range(n)] for i in range(n)]
    out[3] = mp.fsum(mp.fdot(w[i], k[i]) for i in range(n)) / 2
    for c in range(3 * d):
        out[4 + c] = mp.fsum(mp.fdot(w[i], dk[c][i]) for i in range(n)) / 2
    return split(out)


def one(name):
    x, y, ls, lam, period = T.case_inputs(name)
    hi, lo = evaluate(x.numpy(), y.numpy(), [T.NOISE] * x.shape[0], ls.numpy(), lam.numpy(), period.numpy(), T.OUTPUTSCALE, T.MEAN)
    print(name, "done", flush=True)
    return name, hi, lo, T.checksum([x, y, ls, lam, period])


def build(processes=None):
    out = {}
    out["pairs/hi"], out["pairs/lo"] = pairs_table()
    out["pairs/sha256"] = np.array(T.checksum([torch.from_numpy(T.pair_deltas()), T.pair_parameters()]))
    with multiprocessing.Pool(processes) as pool:
        for name, hi, lo, sha in pool.imap_unordered(one, sorted(T.CASES, key=lambda k: -T.CASES[k][0])):
            out[f"{name}/hi"], out[f"{name}/lo"] = hi, lo
            out[f"{name}/case"] = np.array(T.CASES[name], dtype=np.float64)  # n, d, seed
            out[f"{name}/sha256"] = np.array(sha)
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
