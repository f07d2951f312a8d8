"""Host: the Student-t fit of the exact-GP residuals (fit_student_t driven by the CPU helper as ``evaluate``), the averaging
of estimate_student_parameters, the interval of ConformaliseGP, the conformal metrics and the argument checks of
pls_kernel_mean that need no GPU."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import projected_langevin_sampling_amd as pkg
import student_noise_truth as T
from projected_langevin_sampling_amd import metrics
from projected_langevin_sampling_amd.conformalise import ConformalPrediction, gaussian_interval

F64 = torch.float64
L = pkg._lib
FIT_CASES = [(50, 3.0, 0.5), (257, 5.0, 0.3), (1000, 4.0, 1.0), (5000, 8.0, 0.2), (1000, 50.0, 1.0)]


@pytest.mark.parametrize("name", list(T.CASES))
def test_helper_against_50_digits(name):
    """the fsum helper's gradient and Hessian against the mpmath fixture, to 16 eps S"""
    _, nu, s, _ = T.CASES[name]
    d = T.student_derivatives(T.case_inputs(name), nu, s)
    hi, lo = T.truth(name)
    got, mag = (np.array([d[k][i] for k in T.OUTPUTS]) for i in (0, 1))
    err = T.relative_error(got, hi, lo, mag)
    print(f"{name}: |helper - truth| / S per output, in eps: {np.round(err / T.EPS, 3)}")
    assert np.all(err <= 16 * T.EPS)


_fits = {}


def fitted(case):
    if case not in _fits:
        r = T.student_t_samples(*case)
        _fits[case] = (r, pkg.fit_student_t(r, evaluate=T.student_sums))
    return _fits[case]


@pytest.mark.parametrize("case", FIT_CASES, ids=[f"n{n}-nu{nu:g}-s{s:g}" for n, nu, s in FIT_CASES])
def test_fit_is_stationary(case):
    """|g_k| <= 2 (n + 64) eps S_k at the returned point, per component of the gradient in (log nu, log s)"""
    r, (nu, s) = fitted(case)
    assert nu > 0 and s > 0
    for name, (g, bar) in zip(("log nu", "log s"), T.stationarity(r, nu, s)):
        print(f"{case}: nu {nu:.10g} s {s:.10g}  |d ll / d {name}| {g:.2e}, bar {bar:.2e} (ratio {g / bar:.1e})")
        assert g <= bar


@pytest.mark.parametrize("case", FIT_CASES, ids=[f"n{n}-nu{nu:g}-s{s:g}" for n, nu, s in FIT_CASES])
def test_fit_is_no_worse_than_scipy(case):
    """NLL(ours) <= NLL(scipy.stats.t.fit(r, floc=0)) + (n + 64) eps sum|term|: the reference's own optimiser"""
    stats = pytest.importorskip("scipy.stats")
    r, (nu, s) = fitted(case)
    df, _, scale = stats.t.fit(r.numpy(), floc=0)
    ours, mag = T.negative_log_likelihood(r, nu, s)
    theirs, _ = T.negative_log_likelihood(r, float(df), float(scale))
    print(f"{case}: ours ({nu:.8g}, {s:.8g}) scipy ({df:.8g}, {scale:.8g}); NLL ours - scipy {ours - theirs:.2e}")
    assert ours <= theirs + (r.numel() + 64) * T.EPS * mag


def test_gaussian_residuals_end_at_the_bound():
    """1000 standard normals whose sample kurtosis is below 3: the likelihood rises in nu all the way (for a kurtosis
    above 3 a finite maximiser exists even for normal draws, so the seed is one with the premise of this test).  nu ends at
    the upper bound with ONE warning; the scale is sqrt(mean r^2) up to the O(1/nu) = 1e-6 correction."""
    r = torch.randn(1000, generator=torch.Generator().manual_seed(1), dtype=F64)
    assert float((r**4).mean() / (r**2).mean() ** 2) < 3.0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nu, s = pkg.fit_student_t(r, evaluate=T.student_sums)
    assert len(caught) == 1 and "bound" in str(caught[0].message)
    assert abs(nu / 1e6 - 1.0) <= 1e-12
    assert abs(s / math.sqrt(float(r.square().mean())) - 1.0) <= 1e-4
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        nu, _ = pkg.fit_student_t(r, deg_free_bounds=(0.5, 30.0), evaluate=T.student_sums)
    assert len(caught) == 1 and abs(nu / 30.0 - 1.0) <= 1e-12


def test_estimate_student_parameters_averages_the_models():
    y = T.student_t_samples(257, 5.0, 0.3)
    g = torch.Generator().manual_seed(3)
    shifts = [0.05 * torch.randn(257, generator=g, dtype=F64) for _ in range(3)]
    means = [torch.zeros(257, dtype=F64) + sh for sh in shifts]
    want = pkg.fit_student_t(y - (shifts[0] + shifts[1] + shifts[2]) / 3.0, evaluate=T.student_sums)
    got = pkg.estimate_student_parameters(y, means, evaluate=T.student_sums)
    as_tuples = pkg.estimate_student_parameters(y, [(m, None, None) for m in means], evaluate=T.student_sums)
    residuals = torch.stack([y - m for m in means], dim=1).mean(dim=1)
    for (g_k, bar) in T.stationarity(residuals, *got):
        assert g_k <= bar
    assert got == as_tuples
    assert abs(got[0] / want[0] - 1.0) <= 1e-6 and abs(got[1] / want[1] - 1.0) <= 1e-6
    with pytest.raises(ValueError):
        pkg.estimate_student_parameters(y, [], evaluate=T.student_sums)


def test_student_t_likelihood_limit_is_documented():
    assert "2" in pkg.fit_student_t.__doc__ and "StudentTLikelihood" in pkg.fit_student_t.__doc__


@pytest.mark.parametrize("coverage", [0.5, 2 / 3, 0.95])
def test_gaussian_interval_against_scipy(coverage):
    stats = pytest.importorskip("scipy.stats")
    g = torch.Generator().manual_seed(4)
    mean, var = torch.randn(10, generator=g, dtype=F64), torch.rand(10, generator=g, dtype=F64) + 0.1
    z = stats.norm.interval(coverage)[1]
    lower, upper = gaussian_interval(mean, var, coverage)
    half = z * np.sqrt(var.numpy())
    assert np.all(np.abs(upper.numpy() - mean.numpy() - half) <= 4 * T.EPS * half)
    assert np.all(np.abs(mean.numpy() - lower.numpy() - half) <= 4 * T.EPS * half)


def test_conformal_metrics_against_numpy():
    g = torch.Generator().manual_seed(6)
    mean = torch.randn(10, generator=g, dtype=F64)
    half = torch.rand(10, generator=g, dtype=F64) + 0.2
    y = mean + 1.5 * half * torch.randn(10, generator=g, dtype=F64)
    pred = ConformalPrediction(coverage=2 / 3, mean=mean, lower=mean - half, upper=mean + 1.2 * half)
    lo, up, m, yy = (t.numpy() for t in (pred.lower, pred.upper, mean, y))
    std = (up - lo) / 2
    want_nll = np.mean(0.5 * np.log(2 * np.pi * std**2) + (yy - m) ** 2 / (2 * std**2))
    assert abs(metrics.calculate_nll(pred, y) - want_nll) <= 1e-14 * max(1.0, abs(want_nll))
    want_cov = np.mean(((lo <= yy) & (yy <= up)).astype(np.float32))
    assert 0.0 < want_cov < 1.0 and metrics.calculate_coverage(pred, y) == float(want_cov)
    with pytest.raises(AssertionError, match="2/3"):
        metrics.calculate_nll(ConformalPrediction(coverage=0.9, mean=mean, lower=pred.lower, upper=pred.upper), y)
    assert metrics.calculate_mae(pred, y) == (mean - y).abs().mean().item()

    class Model:  # what the width metrics ask of a conformal model
        def predict_coverage(self, x, coverage):
            return pred.lower * coverage, pred.upper * coverage

        def calculate_average_interval_width(self, x, coverage):
            lower, upper = self.predict_coverage(x, coverage)
            return torch.mean(upper - lower).item()

    assert abs(metrics.calculate_average_interval_width(Model(), None, 0.9) - np.mean(0.9 * (up - lo))) <= 1e-15
    assert abs(metrics.calculate_median_interval_width(Model(), None, 0.9) - np.sort(0.9 * up - 0.9 * lo)[4]) <= 1e-15


def test_conformalise_gp_rejects_other_models():
    from projected_langevin_sampling_amd.conformalise import ConformaliseGP, ConformalisePLS, _ConformaliseBase

    x, y = torch.zeros(4, 1, dtype=F64), torch.zeros(4, dtype=F64)
    with pytest.raises(TypeError):
        ConformaliseGP(object(), x, y)
    with pytest.raises(ValueError, match="likelihood"):
        ConformaliseGP(pkg.SVGP(pkg.ARDKernel([1.0], 1.0), x, likelihood=pkg.BernoulliLikelihood()), x, y)
    assert issubclass(ConformaliseGP, _ConformaliseBase) and issubclass(ConformalisePLS, _ConformaliseBase)


def test_kernel_mean_argument_checks():
    """what pls_kernel_mean refuses before anything touches the GPU"""
    lib = L.load()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first, or has nothing to do

    def mean(kind=0, x=p, n=4, d=2, ls=p, alpha=p, xt=p, t=3, out=p):
        return lib.pls_kernel_mean(kind, x, n, d, ls, 1.0, 0.0, alpha, xt, t, out, None), lib.pls_last_error()

    assert mean(d=65)[0] == 1 and b"> 64 is not supported" in mean(d=65)[1]
    assert mean(kind=L.KERNEL_LINEAR)[0] == 1 and b"linear kernel" in mean(kind=L.KERNEL_LINEAR)[1]
    assert mean(kind=5)[0] == 1 and b"unknown kernel kind 5" in mean(kind=5)[1]
    for bad in (dict(n=0), dict(d=0), dict(t=-1)):
        assert mean(**bad)[0] == 1 and b"bad sizes" in mean(**bad)[1], bad
    for name in ("x", "ls", "alpha", "xt", "out"):
        assert mean(**{name: None})[0] == 1 and b"NULL pointer" in mean(**{name: None})[1], name
    assert mean(t=0)[0] == 0, "t == 0 is PLS_OK and launches nothing"
    assert "pls_kernel_mean" in L.SIGNATURES and L.ABI_VERSION == 7
