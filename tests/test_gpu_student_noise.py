"""GPU: the Student-t noise stage of the regression drivers -- ExactGP.predict_mean against LAPACK and against predict, its
alpha cache, fit_student_t and estimate_student_parameters on the device against the CPU helper's stationarity bar, the
hand-over to StudentTCost, and ConformaliseGP over an ExactGP and two SVGPs."""
import numpy as np
import pytest
import torch

import student_noise_truth as T
from matern_closed_form import matern_torch

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _training_data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    y = torch.sin(1.5 * x[:, 0]) + 0.5 * x[:, -1] + 0.2 * torch.randn(n, generator=g, dtype=F64)
    return x, y


def _lapack_mean(kernel_name, model, x, y, xt):
    s, noise, c, ls = model.outputscale, model.noise, model.mean_constant, model.lengthscale
    if kernel_name == "rbf":
        def k(a, b):
            return s * T.cross_kappa(T.RBF, a, b, ls)
    else:
        k = matern_torch(ls, s, 2.5)
    ky = k(x, x) + noise * torch.eye(x.shape[0], dtype=F64)
    assert torch.linalg.cond(ky).item() <= 1e3
    low = torch.linalg.cholesky(ky)
    return c + k(x, xt).T @ torch.cholesky_solve((y - c)[:, None], low)[:, 0]


@pytest.mark.parametrize("kernel", ["matern52", "rbf"])
def test_predict_mean_against_the_helper_and_predict(kernel):
    import projected_langevin_sampling_amd as pkg

    x, y = _training_data(130, 2, 22)
    xt = torch.randn(40, 2, generator=torch.Generator().manual_seed(23), dtype=F64)
    model = pkg.ExactGP(x, y, kernel)
    raw = torch.tensor([0.1, -1.5, 0.3, 0.2, 0.6], dtype=F64)
    model.set_raw_parameters(raw)
    s = model.outputscale
    got = model.predict_mean(xt)
    assert got.shape == (40,) and got.is_cuda
    e_helper = ((got.cpu() - _lapack_mean(kernel, model, x, y, xt)).abs().max() / s).item()
    e_predict = ((got - model.predict(xt)[0]).abs().max() / s).item()
    print(f"{kernel}: predict_mean vs LAPACK {e_helper:.2e}, vs predict {e_predict:.2e} (relative to s)")
    assert e_helper <= 1e-11 and e_predict <= 1e-11
    assert torch.equal(got, model.predict_mean(xt)), "the cached alpha gives other bits"
    # the cache follows the parameters
    other = raw + torch.tensor([0.3, 0.4, -0.2, 0.1, -0.3], dtype=F64)
    model.set_raw_parameters(other)
    moved = model.predict_mean(xt)
    e_moved = ((moved.cpu() - _lapack_mean(kernel, model, x, y, xt)).abs().max() / model.outputscale).item()
    assert e_moved <= 1e-11 and (moved - got).abs().max().item() > 1e-3
    model.set_raw_parameters(raw)
    assert torch.equal(got, model.predict_mean(xt))
    assert model.predict_mean(xt[:0]).shape == (0,)


@pytest.mark.parametrize("case", [(257, 5.0, 0.3), (5000, 8.0, 0.2)], ids=["n257", "n5000"])
def test_fit_student_t_on_the_device(case):
    import projected_langevin_sampling_amd as pkg

    r = T.student_t_samples(*case)
    a, b, c = pkg.gaussian_process.student_t_sums_on_device(r.cuda(), 4.0, 0.5)
    for got, want in zip((a, b, c), T.student_sums(r, 4.0, 0.5)):
        assert abs(got - want) <= 1e-12 * want
    nu, s = pkg.fit_student_t(r.cuda())
    host = pkg.fit_student_t(r, evaluate=T.student_sums)
    for name, (g, bar) in zip(("log nu", "log s"), T.stationarity(r, nu, s)):
        print(f"{case}: device fit nu {nu:.10g} s {s:.10g} (host {host[0]:.10g} {host[1]:.10g}); |d ll / d {name}| {g:.2e}, "
              f"bar {bar:.2e} (ratio {g / bar:.1e})")
        assert g <= bar


def test_estimate_student_parameters_end_to_end():
    """two ExactGPs on 130-point subsamples of 400 points with Student-t noise (nu = 4) predict at all 400 points; the fit
    of their averaged residuals is stationary for the CPU-computed residuals, and feeds a StudentTCost step"""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.basis import OrthonormalBasis
    from projected_langevin_sampling_amd.costs import StudentTCost
    from projected_langevin_sampling_amd.link_functions import IdentityLinkFunction

    x, clean = _training_data(400, 2, 31)
    y = clean + T.student_t_samples(400, 4.0, 0.15, seed=2)
    raws = [torch.tensor([0.1, -1.5, 0.3, 0.2, 0.6], dtype=F64), torch.tensor([0.0, -1.0, 0.1, 0.4, 0.3], dtype=F64)]
    models, cpu_means = [], []
    for k, raw in enumerate(raws):
        idx = torch.arange(k * 135, k * 135 + 130)
        model = pkg.ExactGP(x[idx], y[idx], "matern52").set_raw_parameters(raw)
        models.append(model)
        cpu_means.append(_lapack_mean("matern52", model, x[idx], y[idx], x))
    means = [m.predict_mean(x) for m in models]
    nu, s = pkg.estimate_student_parameters(y, means)
    residuals = torch.stack([y - m for m in cpu_means], dim=1).mean(dim=1)
    for name, (g, bar) in zip(("log nu", "log s"), T.stationarity(residuals, nu, s)):
        print(f"end to end: nu {nu:.8g} s {s:.8g}; |d ll / d {name}| {g:.2e}, bar {bar:.2e}")
        assert g <= bar
    nu2, s2 = pkg.estimate_student_parameters(y, [m.predict(x) for m in models])  # tuples: their first element is used
    assert abs(nu2 / nu - 1.0) <= 1e-6 and abs(s2 / s - 1.0) <= 1e-6
    z = x[:24].clone()
    basis = OrthonormalBasis(pkg.PLSKernel(pkg.construct_average_ard_kernel(models), z), z, x, 1e-6, verbose=False)
    cost = StudentTCost(nu, y, IdentityLinkFunction(), s)
    u = torch.randn(basis.approximation_dimension, 16, generator=torch.Generator().manual_seed(32), dtype=F64)
    update = pkg.PLS(basis, cost).calculate_particle_update(u.cuda(), 1e-3)
    assert update.shape == u.shape and torch.isfinite(update).all()


def _numpy_conformal(predict, student, xc, yc, xs, coverage):
    """conformalise/base.py:58-114 restated on the model's own predict output"""
    from statistics import NormalDist

    z = NormalDist().inv_cdf((1 + coverage) / 2)

    def interval(x):
        mean, latent, obs = (v.cpu().numpy() for v in predict(x))
        half = z * np.sqrt(obs - latent if student else obs)
        return mean - half, mean + half, mean

    lo, up, _ = interval(xc)
    scores = np.maximum(lo - yc.numpy(), yc.numpy() - up)
    n = len(scores)
    q = np.quantile(scores, float(np.clip((n + 1) * coverage / n, 0.0, 1.0)))  # linear interpolation
    lo, up, median = interval(xs)
    return np.minimum(lo - q, median), np.maximum(up + q, median), median


@pytest.mark.parametrize("which", ["exact", "svgp-gaussian", "svgp-student"])
def test_conformalise_gp(which):
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd import metrics

    x, y = _training_data(330, 2, 41)
    xtr, ytr, xc, yc, xs, ys = x[:130], y[:130], x[130:230], y[130:230], x[230:], y[230:]
    if which == "exact":
        gp = pkg.ExactGP(xtr, ytr, "rbf").set_raw_parameters(torch.tensor([0.1, -1.5, 0.3, 0.2, 0.6], dtype=F64))
    else:
        lik = pkg.StudentTLikelihood(4.0) if which == "svgp-student" else None
        gp, losses = pkg.train_svgp(xtr, ytr, xtr[:16].clone(), pkg.ARDKernel([1.0, 1.0], 1.0), 0, 5, 32, 0.01, 1e9, likelihood=lik)
        assert gp is not None and np.all(np.isfinite(losses))
    conf = pkg.ConformaliseGP(gp, xc, yc)
    for coverage in (2 / 3, 0.9):
        lower, upper = conf.predict_coverage(xs, coverage)
        want_lo, want_up, want_med = _numpy_conformal(gp.predict, which == "svgp-student", xc, yc, xs, coverage)
        scale = np.abs(want_up).max() + np.abs(want_lo).max()
        err = max(np.abs(lower.cpu().numpy() - want_lo).max(), np.abs(upper.cpu().numpy() - want_up).max()) / scale
        print(f"{which} coverage {coverage:.3f}: |bounds - numpy| {err:.2e}")
        assert err <= 1e-12
        median = conf.predict_median(xs)
        assert np.array_equal(median.cpu().numpy(), want_med)
        assert bool((lower <= median).all()) and bool((median <= upper).all())
        on_calibration = metrics.calculate_coverage(conf(xc, coverage), yc.cuda())
        assert on_calibration >= coverage - 1e-7, (on_calibration, coverage)  # (a float32 mean)
    pred = conf(xs, 2 / 3)
    assert np.isfinite(metrics.calculate_nll(pred, ys.cuda())) and 0.0 <= metrics.calculate_coverage(pred, ys.cuda()) <= 1.0
    width = metrics.calculate_average_interval_width(conf, xs, 0.9)
    assert width > 0 and metrics.calculate_median_interval_width(conf, xs, 0.9) > 0
    assert torch.equal(conf.predict_variance(xs), (pred.upper - pred.lower) / 2)


def test_conformalise_gp_refuses_a_bernoulli_svgp():
    import projected_langevin_sampling_amd as pkg

    x, y = _training_data(60, 2, 42)
    gp, _ = pkg.train_svgp(x, (y > 0).double(), x[:8].clone(), pkg.ARDKernel([1.0, 1.0], 1.0), 0, 1, 30, 0.01, 1e9,
                           likelihood=pkg.BernoulliLikelihood())
    with pytest.raises(ValueError):
        pkg.ConformaliseGP(gp, x, y)
