"""Writes tests/golden/student_noise_truth.npz: gradient and Hessian in (log nu, log s) of the zero-location Student-t
log-likelihood for the cases of tests/student_noise_truth.py in 50-digit arithmetic (mpmath), stored as hi / lo double
pairs.  The residuals are not stored: the tests regenerate them from the case table and compare their SHA-256 with the
one recorded here.  Offline, seconds:  python tests/golden/make_student_noise_truth.py"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import student_noise_truth as T  # noqa: E402

mp.mp.dps = 50


def evaluate(r, nu, s):
    """(ll_a, ll_b, ll_aa, ll_ab, ll_bb); every float64 input is taken exactly"""
    nu, s = mp.mpf(float(nu)), mp.mpf(float(s))
    n = len(r)
    u = [mp.mpf(float(v)) ** 2 / (nu * s * s) for v in r]
    a = mp.fsum(mp.log1p(v) for v in u)
    b = mp.fsum(v / (1 + v) for v in u)
    c = mp.fsum(v / (1 + v) ** 2 for v in u)
    h1 = (mp.digamma((nu + 1) / 2) - mp.digamma(nu / 2)) / 2 - 1 / (2 * nu)
    h2 = (mp.polygamma(1, (nu + 1) / 2) - mp.polygamma(1, nu / 2)) / 4 + 1 / (2 * nu * nu)
    return [n * nu * h1 - nu * a / 2 + (nu + 1) * b / 2,
            -n + (nu + 1) * b,
            n * nu * (h1 + nu * h2) - nu * a / 2 + nu * b - (nu + 1) * c / 2,
            nu * b - (nu + 1) * c,
            -2 * (nu + 1) * c]


def build():
    out = {}
    for name, (n, nu, s, seed) in T.CASES.items():
        r = T.case_inputs(name)
        vals = evaluate(r.numpy(), nu, s)
        hi = np.array([float(v) for v in vals])
        out[f"{name}/hi"] = hi
        out[f"{name}/lo"] = np.array([float(v - mp.mpf(h)) for v, h in zip(vals, hi)])
        out[f"{name}/case"] = np.array([n, nu, s, seed], dtype=np.float64)
        out[f"{name}/sha256"] = np.array(T.checksum([r]))
    return {k: out[k] for k in sorted(out)}


if __name__ == "__main__":
    np.savez(T.TRUTH, **build())
