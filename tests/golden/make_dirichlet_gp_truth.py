"""Writes tests/golden/dirichlet_gp_truth.npz: per class the exact-GP marginal log-likelihood and its gradient (a row of
pls_gp_mll_grad_classes) for the cases of tests/dirichlet_gp_truth.py, in 50-digit arithmetic (mpmath) with the diagonal
v_c + sigma_c, stored as hi / lo double pairs.  The inputs are not stored: the tests regenerate them from the case table
and compare their SHA-256 with the one recorded here.  Offline, a few minutes on a few cores:
python tests/golden/make_dirichlet_gp_truth.py"""
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import dirichlet_gp_truth as T  # noqa: E402
from make_exact_gp_truth import kernel_and_derivatives  # noqa: E402

mp.mp.dps = 50


def evaluate(kind, x, y, diag, ls, s, mean):
    """one class; every float64 input is taken exactly"""
    n, d = x.shape
    s, mean = mp.mpf(float(s)), mp.mpf(float(mean))
    k, dk = kernel_and_derivatives(kind, x, ls, s)
    a = [[k[i][j] + (mp.mpf(float(diag[i])) if i == j else 0) for j in range(n)] for i in range(n)]
    low = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for c in range(i):
            low[i][c] = (a[i][c] - mp.fdot(low[i][:c], low[c][:c])) / low[c][c]
        low[i][i] = mp.sqrt(a[i][i] - mp.fdot(low[i][:i], low[i][:i]))
    cols = [[mp.mpf(0)] * n for _ in range(n)]  # cols[c][i] = Linv[i][c], Linv = Lc^-1
    for c in range(n):
        col = cols[c]
        for i in range(c, n):
            col[i] = ((1 if i == c else 0) - mp.fdot(low[i][c:i], col[c:i])) / low[i][i]
    p = [[mp.mpf(0)] * n for _ in range(n)]  # P = K_y^-1 = Linv^T Linv
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
    out[3] = mp.fsum(mp.fdot(w[i], k[i]) for i in range(n)) / 2
    for c in range(d):
        out[4 + c] = mp.fsum(mp.fdot(w[i], dk[c][i]) for i in range(n)) / 2
    hi = np.array([float(v) for v in out])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(out, hi)])
    return hi, lo


def one(job):
    name, c = job
    kind, x, _, y, v, ls, s, sigma, mean = T.case_inputs(name)
    diag = (v[c] + sigma[c]).numpy()  # the float64 sum the device forms as well (jitter 0)
    hi, lo = evaluate(kind, x.numpy(), y[c].numpy(), diag, ls[c].numpy(), s[c].item(), mean[c].item())
    print(name, "class", c, "done", flush=True)
    return name, c, hi, lo


def build(names=None, processes=None):
    names = sorted(names or T.CASES, key=lambda k: -T.CASES[k][1])  # the largest first
    jobs = [(name, c) for name in names for c in range(T.CASES[name][3])]
    rows = {}
    with multiprocessing.Pool(processes) as pool:
        for name, c, hi, lo in pool.imap_unordered(one, jobs):
            rows[name, c] = (hi, lo)
    out = {}
    for name in names:
        classes = T.CASES[name][3]
        out[f"{name}/hi"] = np.stack([rows[name, c][0] for c in range(classes)])
        out[f"{name}/lo"] = np.stack([rows[name, c][1] for c in range(classes)])
        out[f"{name}/case"] = np.array(T.CASES[name], dtype=np.float64)  # kind, n, d, classes, seed
        out[f"{name}/sha256"] = np.array(T.checksum(*T.case_inputs(name)[1:]))
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
