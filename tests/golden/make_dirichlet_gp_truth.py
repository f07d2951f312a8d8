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
from make_exact_gp_truth import evaluate  # noqa: E402

mp.mp.dps = 50


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
        out[f"{name}/sha256"] = np.array(T.checksum(T.case_inputs(name)[1:]))
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
