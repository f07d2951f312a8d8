"""Writes tests/golden/svgp_quadrature_truth.npz: the output vector of tests/svgp_quadrature_truth.py (ELBO, d/dc, d/drho, mean
log-likelihood, KL, d/dm, the lower triangle of d/dL_s) for its fixture cases and likelihoods in 50-digit arithmetic
(mpmath), stored as hi / lo double pairs.  The Gauss-Hermite nodes and weights are the DOUBLES of the truth module's
tables, taken exactly: the quadrature sum is the contract, not the integral.  The inputs are not stored: the tests
regenerate them from the case table and compare their SHA-256 with the one recorded here.  Offline, a few minutes:
python tests/golden/make_svgp_quadrature_truth.py"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import svgp_quadrature_truth as QT  # noqa: E402
import svgp_truth as T  # noqa: E402

mp.mp.dps = 50
X = [mp.mpf(float(v)) for v in QT.GH_X]
W = [mp.mpf(float(v)) for v in QT.GH_W]


def node(lik, nu, y, f, sig2):
    """(g, g', dg/ds2) at one node"""
    if lik == QT.BERNOULLI:
        s = 2 * y - 1
        z = s * f
        cdf = mp.erfc(-z / mp.sqrt(2)) / 2
        return mp.log(cdf), s * mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) / cdf, mp.mpf(0)
    r = y - f
    d = nu * sig2 + r * r
    g = (mp.loggamma((nu + 1) / 2) - mp.loggamma(nu / 2) - mp.log(nu * mp.pi * sig2) / 2
         - (nu + 1) / 2 * mp.log(1 + r * r / (nu * sig2)))
    return g, (nu + 1) * r / d, -1 / (2 * sig2) + (nu + 1) * r * r / (2 * sig2 * d)


def evaluate(lik, nu, inp):
    f = lambda t: [mp.mpf(float(v)) for v in t]  # noqa: E731  (float64 inputs, taken exactly)
    nu = mp.mpf(nu)
    idx = inp["idx"].tolist()
    a = [f(inp["At"][i]) for i in idx]
    q, y = f(inp["q"][idx]), f(inp["y"][idx])
    mean = f(inp["mean"])
    m, b, n = len(mean), len(idx), inp["n"]
    low = [f(row) for row in inp["Ls"]]
    c, rho = mp.mpf(inp["c"]), mp.mpf(inp["rho"])
    sig2 = mp.log(1 + mp.exp(rho))  # (no floor)
    mu = [c + mp.fdot(a[i], mean) for i in range(b)]
    w = [[mp.fdot(a[i][l:], [low[p][l] for p in range(l, m)]) for l in range(m)] for i in range(b)]
    ell, gmu, gv, ds = [], [], [], []
    for i in range(b):
        sq = mp.sqrt(2 * (q[i] + mp.fdot(w[i], w[i])))
        terms = [node(lik, nu, y[i], mu[i] + sq * X[k], sig2) for k in range(QT.Q)]
        ell.append(mp.fsum(W[k] * terms[k][0] for k in range(QT.Q)))
        gmu.append(mp.fsum(W[k] * terms[k][1] for k in range(QT.Q)))
        gv.append(mp.fsum(W[k] * X[k] * terms[k][1] for k in range(QT.Q)) / sq)
        ds.append(mp.fsum(W[k] * terms[k][2] for k in range(QT.Q)))
    kl = (mp.fsum(low[k][l] ** 2 for k in range(m) for l in range(k + 1)) + mp.fdot(mean, mean) - m
          - 2 * mp.fsum(mp.log(abs(low[p][p])) for p in range(m))) / 2
    grho = mp.fsum(ds) / (1 + mp.exp(-rho)) / b if lik == QT.STUDENT_T else mp.mpf(0)
    out = [mp.fsum(ell) / b - kl / n, mp.fsum(gmu) / b, grho, mp.fsum(ell) / b, kl]
    out += [mp.fsum(gmu[i] * a[i][k] for i in range(b)) / b - mean[k] / n for k in range(m)]
    for k in range(m):
        for l in range(k + 1):
            pen = low[k][l] - (1 / low[k][k] if k == l else 0)
            out.append(2 * mp.fsum(gv[i] * a[i][k] * w[i][l] for i in range(b)) / b - pen / n)
    hi = np.array([float(v) for v in out])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(out, hi)])
    return hi, lo


def build():
    out = {}
    for lik_name, (lik, nu) in QT.LIKELIHOODS.items():
        for name in sorted(QT.CASES):
            inp = QT.case_inputs(lik_name, name)
            key = f"{lik_name}/{name}"
            out[f"{key}/hi"], out[f"{key}/lo"] = evaluate(lik, nu, inp)
            out[f"{key}/sha256"] = np.array(T.checksum(T.hashed(inp)))
            print(key, "done", flush=True)
    return out


if __name__ == "__main__":
    np.savez(QT.TRUTH, **build())
