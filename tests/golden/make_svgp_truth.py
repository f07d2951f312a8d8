"""Writes tests/golden/svgp_truth.npz: the output vector of tests/svgp_truth.py (ELBO, d/dc, d/drho, mean log-likelihood,
KL, d/dm, the lower triangle of d/dL_s) for its fixture cases in 50-digit arithmetic (mpmath), stored as hi / lo double
pairs.  The inputs are not stored: the tests regenerate them from the case table and compare their SHA-256 with the one
recorded here.  Offline, under a minute:  python tests/golden/make_svgp_truth.py"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import svgp_truth as T  # noqa: E402

mp.mp.dps = 50


def evaluate(inp):
    f = lambda t: [mp.mpf(float(v)) for v in t]  # noqa: E731  (float64 inputs, taken exactly)
    idx = inp["idx"].tolist()
    a = [f(inp["At"][i]) for i in idx]
    q, y = f(inp["q"][idx]), f(inp["y"][idx])
    mean = f(inp["mean"])
    m, b, n = len(mean), len(idx), inp["n"]
    low = [f(row) for row in inp["Ls"]]
    c, rho = mp.mpf(inp["c"]), mp.mpf(inp["rho"])
    sig2 = mp.log(1 + mp.exp(rho)) + mp.mpf(T.MIN_NOISE)
    mu = [c + mp.fdot(a[i], mean) for i in range(b)]
    w = [[mp.fdot(a[i][l:], [low[p][l] for p in range(l, m)]) for l in range(m)] for i in range(b)]
    e = [(y[i] - mu[i]) ** 2 + q[i] + mp.fdot(w[i], w[i]) for i in range(b)]
    ell = [-mp.log(2 * mp.pi) / 2 - mp.log(sig2) / 2 - e[i] / (2 * sig2) for i in range(b)]
    gmu = [(y[i] - mu[i]) / sig2 for i in range(b)]
    gv = -1 / (2 * sig2)
    kl = (mp.fsum(low[k][l] ** 2 for k in range(m) for l in range(k + 1)) + mp.fdot(mean, mean) - m
          - 2 * mp.fsum(mp.log(abs(low[p][p])) for p in range(m))) / 2
    out = [mp.fsum(ell) / b - kl / n, mp.fsum(gmu) / b,
           mp.fsum(gv + e[i] / (2 * sig2 * sig2) for i in range(b)) / (1 + mp.exp(-rho)) / b, mp.fsum(ell) / b, kl]
    out += [mp.fsum(gmu[i] * a[i][k] for i in range(b)) / b - mean[k] / n for k in range(m)]
    for k in range(m):
        for l in range(k + 1):
            pen = low[k][l] - (1 / low[k][k] if k == l else 0)
            out.append(2 * mp.fsum(gv * a[i][k] * w[i][l] for i in range(b)) / b - pen / n)
    hi = np.array([float(v) for v in out])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(out, hi)])
    return hi, lo


def build():
    out = {}
    for name in sorted(T.CASES):
        inp = T.case_inputs(name)
        out[f"{name}/hi"], out[f"{name}/lo"] = evaluate(inp)
        out[f"{name}/sha256"] = np.array(T.checksum(T.hashed(inp)))
        print(name, "done", flush=True)
    return out


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
