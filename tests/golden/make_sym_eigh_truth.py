"""Writes tests/golden/sym_eigh_truth.npz: for every family of tests/sym_eigh_truth.py and M in FIXTURE_SIZES the lower
triangle of the float64 matrix and its eigenvalues from mpmath.eigsy at 50 digits, rounded to float64 (ascending).  The
`doubled` family is diag(B, B): B alone goes through mpmath and its eigenvalues are repeated.  About two minutes.
    python tests/golden/make_sym_eigh_truth.py"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sym_eigh_truth as T  # noqa: E402

mp.mp.dps = 50


def mp_eigenvalues(a):
    if a.shape[0] == 0:
        return np.zeros(0)
    lam = mp.eigsy(mp.matrix(a.tolist()), eigvals_only=True)
    return np.sort(np.array([float(v) for v in lam]))


def main():
    out = {}
    for family in T.FAMILIES:
        for m in T.FIXTURE_SIZES:
            a = T.make_matrix(family, m)
            assert np.array_equal(a, a.T)
            if family == "doubled":
                h = m // 2
                lam = np.repeat(mp_eigenvalues(a[:h, :h]), 2)
                if m % 2:
                    lam = np.append(lam, a[m - 1, m - 1])
                lam = np.sort(lam)
            else:
                lam = mp_eigenvalues(a)
            out[f"{family}_{m}_tril"] = a[np.tril_indices(m)]
            out[f"{family}_{m}_lam"] = lam
            print(family, m, "max |lam - LAPACK| / (eps ||A||_2) = %.2f" % (np.abs(lam - np.linalg.eigvalsh(a)).max() / (T.EPS * np.abs(lam).max())), flush=True)
    np.savez_compressed(T.GOLDEN, **out)
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
