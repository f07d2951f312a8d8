"""CPU: the yardstick of the quadrature-likelihood SVGP (tests/svgp_quadrature_truth.py) against its 50-digit fixture and
against autograd of its torch version, its tails, the Python-side validation of the likelihood objects and the new
descriptor's layout and the C ABI's rejections (all before any HIP call)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import svgp_quadrature_truth as QT
import svgp_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(lik, name) for lik in QT.LIKELIHOODS for name in sorted(QT.CASES)]


def test_the_node_table_is_hermgauss_20():
    x, w = np.polynomial.hermite.hermgauss(QT.Q)
    assert np.abs(QT.GH_X - x).max() <= 4 * T.EPS * np.abs(x).max() and (np.abs(QT.GH_OMEGA - w) <= 8 * T.EPS * w).all()
    assert (np.abs(QT.GH_W - QT.GH_OMEGA / math.sqrt(math.pi)) <= 2 * T.EPS * QT.GH_W).all()  # (rounded once: within 2 roundings)
    assert (QT.GH_X == -QT.GH_X[::-1]).all() and (QT.GH_W == QT.GH_W[::-1]).all()
    assert abs(math.fsum(QT.GH_W) - 1.0) <= 2 * T.EPS
    for v in np.concatenate([QT.GH_X, QT.GH_OMEGA, QT.GH_W]):
        assert float(f"{v:.17g}") == v


@pytest.mark.parametrize("lik,name", CASES)
def test_float64_evaluation_against_the_50_digit_truth(lik, name):
    _, out, scale = QT.cpu_case(lik, name)
    m, b, _ = QT.CASES[name]
    hi, lo = QT.truth(lik, name)
    assert hi.shape == out.shape == (5 + m + m * (m + 1) // 2,)
    err = T.relative_error(out, hi, lo, scale)
    print(f"{lik} {name}: worst |fsum - truth| / S = {err.max():.2e}, bar {T.bar(m, b):.2e}")
    assert np.isfinite(out).all() and (scale >= np.abs(out)).all()
    assert (err <= T.bar(m, b)).all()
    if QT.LIKELIHOODS[lik][0] == QT.BERNOULLI:
        assert out[2] == 0.0 and hi[2] == 0.0


def test_the_allowance_comes_from_the_helper_and_the_fixture():
    worst, c = QT.epilogue_allowance()
    print(f"fsum helper against the fixture: worst {worst:.2f} eps S; c = {c:.1f}")
    assert c == max(16.0, 16.0 * worst) and worst < 16.0


@pytest.mark.parametrize("lik,name", CASES)
def test_hand_derived_gradients_equal_autograd(lik, name):
    inp, out, scale = QT.cpu_case(lik, name)
    m, b, _ = QT.CASES[name]
    code, nu = QT.LIKELIHOODS[lik]
    c, rho = torch.tensor(inp["c"], dtype=torch.float64), torch.tensor(inp["rho"], dtype=torch.float64)
    elbo, g_m, g_l, g_c, g_rho = QT.gradients_autograd(code, nu, inp["At"], inp["q"], inp["y"], inp["mean"], inp["Ls"], c, rho,
                                                       inp["idx"], inp["n"])
    got = np.concatenate([[elbo.item(), g_c.item(), g_rho.item()], g_m.numpy(), T.lower_entries(g_l.numpy())])
    want = np.concatenate([out[:3], out[5:]])
    s = np.concatenate([scale[:3], scale[5:]])
    err = T.relative_error(got, want, np.zeros_like(want), s)
    print(f"{lik} {name}: worst |hand - autograd| / S = {err.max():.2e}, bar {QT.bar(m, b):.2e}")
    assert (err <= QT.bar(m, b)).all()


def test_the_helper_stays_finite_in_the_tails():
    """log Phi and phi / Phi far below where Phi underflows (z = -38), against their asymptotic series
    log Phi(z) = -z^2/2 - log(-z sqrt(2 pi)) + log(1 - 1/z^2 + 3/z^4 - ...),  phi / Phi = -z / (1 - 1/z^2 + 3/z^4 - ...);
    and the M = 256 shape of the device test does reach s f < -100"""
    z = np.array([-40.0, -110.0, -500.0, -3000.0])
    series = 1.0 - 1.0 / z**2 + 3.0 / z**4 - 15.0 / z**6
    want_log = -0.5 * z * z - np.log(-z * math.sqrt(2.0 * math.pi)) + np.log(series)
    assert np.isfinite(QT.log_ndtr(z)).all() and (np.abs(QT.log_ndtr(z) / want_log - 1.0) <= 1e-9).all()
    assert (np.abs(QT.hazard(z) / (-z / series) - 1.0) <= 1e-9).all()
    assert abs(QT.log_ndtr(np.array(0.0)) - math.log(0.5)) <= T.EPS and QT.log_ndtr(np.array(40.0)) == 0.0
    inp = QT.with_targets("bernoulli", T.make_inputs(810000 + 1000 * 256 + 65, 300, 256, 65))
    a, low = inp["At"][inp["idx"]].numpy(), np.tril(inp["Ls"].numpy())
    mu = inp["c"] + a @ inp["mean"].numpy()
    v = inp["q"][inp["idx"]].numpy() + ((a @ low) ** 2).sum(axis=1)
    sf = (2.0 * inp["y"][inp["idx"]].numpy() - 1.0)[:, None] * (mu[:, None] + np.sqrt(2.0 * v)[:, None] * QT.GH_X[None, :])
    print(f"M = 256: min s f = {sf.min():.1f}")
    assert sf.min() < -100.0
    out = QT.evaluate_inputs("bernoulli", inp)
    assert np.isfinite(out).all()


def test_likelihood_objects_validate_on_the_host():
    import projected_langevin_sampling_amd as pkg

    z = torch.zeros(4, 2)
    kernel = pkg.ARDKernel([1.0, 1.0], 1.0)
    for bad in (2.0, 1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="deg_free"):
            pkg.StudentTLikelihood(bad)
    with pytest.raises(ValueError, match="noise must exceed 0.0"):
        pkg.StudentTLikelihood(3.0, noise=0.0)
    with pytest.raises(ValueError, match="noise must exceed 0.0001"):
        pkg.GaussianLikelihood(noise=1e-4)
    with pytest.raises(AttributeError, match="no noise"):
        pkg.SVGP(kernel, z, likelihood=pkg.BernoulliLikelihood(), noise=0.1)
    with pytest.raises(AttributeError, match="no noise"):
        pkg.SVGP(kernel, z, likelihood=pkg.BernoulliLikelihood()).noise
    with pytest.raises(AttributeError, match="no noise"):
        pkg.train_svgp(torch.zeros(8, 2), torch.zeros(8), z, kernel, 0, 1, 4, 0.1, 1e-4, likelihood_noise=0.1,
                       likelihood=pkg.BernoulliLikelihood())
    with pytest.raises(AttributeError, match="no noise"):
        pkg.train_svgp_runner(torch.zeros(8, 2), torch.zeros(8), z, kernel, 0, 1, 4, 0.1, 0.01, 2, 1e-4, observation_noise=0.1,
                              likelihood=pkg.BernoulliLikelihood())
    with pytest.raises(AttributeError, match="BernoulliLikelihood only"):
        pkg.SVGP(kernel, z, likelihood=pkg.StudentTLikelihood(3.0)).predict_proba(z)
    for labels in (torch.tensor([0.0, 1.0, 2.0, 1.0]), torch.tensor([0.0, 0.5, 1.0, 1.0]), torch.tensor([-1.0, 1.0, 1.0, 1.0])):
        with pytest.raises(ValueError, match=r"labels in \{0, 1\}"):
            pkg.SVGP(kernel, z, likelihood=pkg.BernoulliLikelihood()).fit_data(z, labels)
    # the starting raw noise: Student-t has no floor
    model = pkg.SVGP(kernel, z, likelihood=pkg.StudentTLikelihood(4.5), noise=0.3)
    assert abs(T.softplus(model._start[2]) - 0.3) <= 1e-15
    model = pkg.SVGP(kernel, z, likelihood=pkg.StudentTLikelihood(4.5, noise=0.2))
    assert abs(T.softplus(model._start[2]) - 0.2) <= 1e-15
    model = pkg.SVGP(kernel, z, likelihood=pkg.GaussianLikelihood(), noise=0.3)
    assert abs(T.softplus(model._start[2]) + 1e-4 - 0.3) <= 1e-15
    # strings keep their behaviour
    for likelihood in ("bernoulli", "student_t"):
        with pytest.raises(NotImplementedError, match="only 'gaussian'"):
            pkg.SVGP(kernel, z, likelihood=likelihood)
    assert pkg.SVGP(kernel, z).likelihood == "gaussian"


def test_the_descriptor_layout(tmp_path):
    """sizeof and offsets of pls_svgp_lik_desc, and as gcc lays the header's struct out where there is a gcc"""
    import shutil
    import subprocess

    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    assert ctypes.sizeof(L.SvgpLikDesc) == 64 and L.SvgpLikDesc.base.offset == 0 and L.SvgpLikDesc.deg_free.offset == 56
    assert ctypes.sizeof(L.SvgpDesc) == 56 and L.SvgpDesc.likelihood.offset == 48
    assert (L.SVGP_GAUSSIAN, L.SVGP_BERNOULLI, L.SVGP_STUDENT_T) == (0, 1, 2)
    if shutil.which("gcc") is None:
        return
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "plship.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d %d %d\\n", sizeof(pls_svgp_lik_desc), offsetof(pls_svgp_lik_desc, base),\n'
                   '         offsetof(pls_svgp_lik_desc, deg_free), PLS_SVGP_GAUSSIAN, PLS_SVGP_BERNOULLI, PLS_SVGP_STUDENT_T);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [64, 0, 56, 0, 1, 2]


def test_cabi_rejects_before_any_hip_call():
    """an unknown likelihood, a Student-t deg_free that is not > 2 or not finite, what the SVGP entries already reject, a
    short workspace -- on a machine without a GPU, so nothing was launched"""
    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    lib = L.load()

    def desc(likelihood, deg_free=0.0, m=8):
        d = L.SvgpLikDesc()
        d.base.At, d.base.ldat, d.base.q, d.base.y, d.base.n, d.base.m, d.base.likelihood = 8, m, 8, 8, 64, m, likelihood
        d.deg_free = deg_free
        return d

    def grad(d, ws_bytes=1 << 30):
        return lib.pls_svgp_lik_elbo_grad(ctypes.byref(d), 8, 8, d.base.m, 8, None, 64, 8, 8, 8, d.base.m, 8, ws_bytes, None)

    def epoch(d, ws_bytes=1 << 30):
        return lib.pls_svgp_lik_sgd_epoch(ctypes.byref(d), 8, 8, d.base.m, 8, 8, 16, 0.1, 3, 8, 8, ws_bytes, None)

    def predict(d):
        return lib.pls_svgp_lik_predict(ctypes.byref(d), 8, 8, 8, 8, 8, 8, 8, 4, 8, 8, 8, None, None)

    for call in (grad, epoch, predict):
        for code in (3, -1, 17):
            assert call(desc(code)) == 1 and b"unknown likelihood" in lib.pls_last_error()
        for nu in (2.0, 1.0, -3.0, float("nan"), float("inf")):
            assert call(desc(L.SVGP_STUDENT_T, nu)) == 1 and b"deg_free > 2" in lib.pls_last_error()
    for code, nu in ((L.SVGP_GAUSSIAN, 0.0), (L.SVGP_BERNOULLI, 0.0), (L.SVGP_STUDENT_T, 3.0)):
        assert grad(desc(code, nu, m=257)) == 1 and b"257 inducing points > 256" in lib.pls_last_error()
        assert grad(desc(code, nu), ws_bytes=16) == 3 and b"needed" in lib.pls_last_error()
        assert epoch(desc(code, nu), ws_bytes=16) == 3 and b"needed" in lib.pls_last_error()
    assert lib.pls_svgp_lik_elbo_grad(None, 8, 8, 8, 8, None, 64, 8, 8, 8, 8, 8, 1 << 30, None) == 1
    # the Gaussian-only entries keep their message
    d = desc(L.SVGP_BERNOULLI)
    assert lib.pls_svgp_elbo_grad(ctypes.byref(d.base), 8, 8, 8, 8, None, 64, 8, 8, 8, 8, 8, 1 << 30, None) == 1
    assert b"PLS_SVGP_GAUSSIAN only" in lib.pls_last_error()
