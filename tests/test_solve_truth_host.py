"""CPU: the high-precision truth of tests/test_gpu_solve_accuracy.py.  tests/golden/solve_truth.npz matches the matrices this
machine regenerates (checksum) and the 50-digit solve recomputed for the M = 64 cases; the iterative refinement that serves
M = 1024 reproduces the stored truth where both exist, and is accepted (last correction < 1e-3 of LAPACK's forward error) in
every M = 1024 bucket; the residual behind it is exact to doubled precision; the bound is the one the tests state."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import solve_fixtures as F


def test_the_truth_file_covers_the_stored_cases_and_stays_small():
    file = F.load_truth()
    assert sorted({k.rsplit("/", 1)[0] for k in file}) == sorted(F.STORED)
    assert os.path.getsize(F.TRUTH) < 512 * 1024
    for name in F.STORED:
        assert np.array_equal(file[f"{name}/case"], np.array(F.CASES[name], dtype=np.float64)), name
        k, u, truth = F.truth_of(name, file)  # (asserts the checksum)
        assert truth.shape == u.shape and np.abs(file[f"{name}/lo"]).max() <= np.abs(file[f"{name}/hi"]).max() * 2.0 ** -52


@pytest.mark.parametrize("name", [n for n in F.STORED if F.CASES[n][0] == 64])
def test_the_stored_truth_is_what_the_generator_computes(name):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_solve_truth", os.path.join(F.HERE, "golden", "make_solve_truth.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    file, fresh = F.load_truth(), maker.build([name])
    for key, value in fresh.items():
        assert np.array_equal(file[key], value), key


@pytest.mark.parametrize("name", F.STORED)
def test_refinement_reproduces_the_stored_truth(name):
    k, u, truth = F.truth_of(name)
    refined, accept = F.refined_truth(k, u)
    assert accept < 1e-3
    rel = np.linalg.norm((refined - truth).astype(np.float64), axis=0) / np.linalg.norm(truth.astype(np.float64), axis=0)
    lapack = F.errors(k, u, F.host_lapack(torch.linalg.cholesky(k), u), truth)[0]
    assert (rel < 1e-6 * lapack).all(), f"{name}: refined against 50-digit truth {rel}, LAPACK's forward error {lapack}"


@pytest.mark.parametrize("name", F.REFINED)
def test_refinement_is_accepted_at_m_1024(name):
    k, z = F.gram(name)
    u = F.rhs(name, k, z)
    truth, accept = F.refined_truth(k, u)
    assert accept < 1e-3, f"{name}: last correction {accept:.1e} of LAPACK's forward error"
    lc = torch.linalg.cholesky(k)
    cond = torch.linalg.cond(k).item()
    fw, bw = F.errors(k, u, F.host_lapack(lc, u), truth)
    assert (bw < 1024 * 2.0 ** -53).all() and (fw < cond * 1024 * 2.0 ** -53).all(), (fw, bw)  # backward stable
    fwp, _ = F.errors(k, u, F.host_products(lc, u), truth)
    assert (fwp < cond * 1024 * 2.0 ** -53).all(), fwp


def test_the_gram_matrices_are_the_rbf_kernel_and_land_in_their_buckets():
    """exp_reproducible in place of torch.exp: the oracle's kernel to a few ulp, with cond(k(Z,Z)) where the case names say"""
    from oracle import pls_oracle as O

    for name, (m, d, seed, factor, jitter) in F.CASES.items():
        k, z = F.gram(name)
        ls = factor * (0.5 + torch.arange(d, dtype=torch.float64) / (d - 1))
        want = O.RBFARDKernel(ls, F.OUTPUTSCALE)(z, z) + jitter * torch.eye(m, dtype=torch.float64)
        # (a few ulp of exp itself, and of its argument: up to 200 half-squared distances deep in the tail)
        assert (k - want).abs().max() < 2e-15 and ((k - want).abs() / want).max() < 1e-13, name
        assert torch.equal(k, k.T)
        cond = torch.linalg.cond(k - jitter * torch.eye(m, dtype=torch.float64)).item()
        target = {"cond1e4": 1e4, "cond1e8": 1e8, "cond1e12j": 1e12}[name.split("/")[1]]
        assert target / 2 < cond < target * 2, (name, cond)
        if jitter:  # ... which no factorisation survives without the jitter of the schedule
            assert 1e9 < torch.linalg.cond(k).item() < 1e12, name


def _exact(x):
    """a longdouble as a Fraction (hi + lo doubles)"""
    hi = x.astype(np.float64)
    return Fraction(float(hi)) + Fraction(float((x - hi).astype(np.float64)))


def test_the_residual_is_exact_to_doubled_precision():
    g = torch.Generator().manual_seed(0)
    n = 40
    k = torch.randn(n, n, generator=g, dtype=torch.float64).numpy().astype(np.longdouble)
    x = torch.randn(n, 3, generator=g, dtype=torch.float64).numpy().astype(np.longdouble) * (1 + np.longdouble(2.0) ** -60)
    u = (k @ x).astype(np.float64).astype(np.longdouble)
    got = F.residual(k, x, u)
    scale = float(np.abs(k).sum(axis=1).max() * np.abs(x).max())
    for i in range(n):
        for c in range(3):
            want = _exact(u[i, c]) - sum(_exact(k[i, t]) * _exact(x[t, c]) for t in range(n))
            assert abs(_exact(got[i, c]) - want) < scale * 2.0 ** -62 * max(abs(want) / scale, 2.0 ** -40), (i, c)


def test_within_is_the_bound_the_tests_state():
    host = np.array([1e-16, 1e-12, 1e-12, 1e-12])
    ok, ratio = F.within(np.array([7e-12, 7e-12, 7e-12, 7e-12]), host, 64)
    assert ok and abs(ratio - 7.0) < 1e-9  # the first column leans on the median
    assert not F.within(np.array([1e-16, 9e-12, 1e-12, 1e-12]), host, 64)[0]
    assert F.within(np.array([8 * 64 * 2.0 ** -53] * 4), np.zeros(4), 64)[0]
