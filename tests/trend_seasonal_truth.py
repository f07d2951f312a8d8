"""The yardstick of the trend-plus-seasonal exact-GP tests, modelled on locally_periodic_truth.py: the closed-form kernel and
its derivatives, the 4 d + 2 pair sums of pls_kernel_grad_sums, and the marginal log-likelihood with its 4 + 4 d + 1 derivatives
through LAPACK -- float64 on the CPU, sums by math.fsum -- together with the tables of tests/golden/trend_seasonal_truth.npz
(50-digit values, written by tests/golden/make_trend_seasonal_truth.py).

With delta_k = x_ik - x_jk, kappa_t = exp(-1/2 sum_k (delta_k / l_k)^2), kappa_s the locally periodic kappa of (m, lambda, p) and
K = s_t kappa_t + s_s kappa_s:
    dK / d log s_t      = s_t kappa_t
    dK / d log l_k      = s_t kappa_t (delta_k / l_k)^2
    dK / d log m_k      = s_s kappa_s (delta_k / m_k)^2
    dK / d log lambda_k = s_s kappa_s (2 / lambda_k) sin^2(pi e_k)
    dK / d log p_k      = s_s kappa_s (2 / lambda_k) pi e_k sin(2 pi e_k)
    dK / d log s_s      = s_s kappa_s
A term whose kappa is 0 contributes 0 to its sums."""
import math
import os

import numpy as np
import torch

from exact_gp_truth import EPS, MEAN, NOISE, fsum_rows  # noqa: F401
from locally_periodic_truth import draw_parameters as seasonal_parameters
from trend_seasonal_closed_form import sensitivity, trend_seasonal_factors_numpy, trend_sensitivity
from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

TREND_SEASONAL = 12  # pls_kernel_kind
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trend_seasonal_truth.npz")
S_T, S_S = 2.5, 0.9


def _np(v):
    return (v.detach().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64))


def factors(x, ls, env, lam, period):
    """(kappa_t (n, n), ft (n, n, d), kappa_s (n, n), fe, fl, fp, e (n, n, d) each, delta (n, n, d)) of all pairs of x, numpy"""
    x = _np(x)
    x = x if x.ndim == 2 else x[:, None]
    delta = x[:, None, :] - x[None, :, :]
    return trend_seasonal_factors_numpy(delta, _np(ls), _np(env), _np(lam), _np(period)) + (delta,)


def gram(x, ls, env, lam, period, s_t, s_s):
    f = factors(x, ls, env, lam, period)
    return torch.from_numpy(float(s_t) * f[0] + float(s_s) * f[2])


def pair_terms(x, ls, env, lam, period, s_t, s_s, alpha, p, majorant=False):
    """(4 d + 2, n, n): the terms of the sums in the library's order -- W kappa_t, W dK / d log l_k, W dK / d log m_k, W dK / d log
    lambda_k, W dK / d log p_k, W s_s kappa_s -- with W = alpha alpha^T - P.  ``majorant``: instead of each term what bounds its
    first-order error budget: its magnitude (the period term with |sin(2 pi e)| replaced by 1) times the sensitivity of its own
    exponent, c_t = 1 + r_t^2 for the trend's terms (trend_seasonal_closed_form.trend_sensitivity), c_s for the seasonal ones
    (locally_periodic_closed_form.sensitivity)."""
    w = _np(alpha)[:, None] * _np(alpha)[None, :] - _np(p)
    kap_t, ft, kap_s, fe, fl, fp, e, delta = factors(x, ls, env, lam, period)
    lam = _np(lam).reshape(-1)
    d = lam.size
    if majorant:
        at = np.abs(w) * kap_t * trend_sensitivity(delta, _np(ls))
        a_s = np.abs(w) * (s_s * kap_s) * sensitivity(delta, e, _np(env), lam)
        per = (2.0 / lam) * np.pi * np.abs(e)
        terms = ([at] + [at * s_t * ft[..., k] for k in range(d)] + [a_s * f[..., k] for f in (fe, fl, per) for k in range(d)] +
                 [a_s])
    else:
        wt = np.where(kap_t == 0.0, 0.0, w * kap_t)
        ws = np.where(kap_s == 0.0, 0.0, w * (s_s * kap_s))
        with np.errstate(invalid="ignore", over="ignore"):  # (a dead term's factors may be inf: its terms are selected to 0)
            terms = ([wt] + [np.where(kap_t == 0.0, 0.0, wt * (s_t * ft[..., k])) for k in range(d)] +
                     [np.where(kap_s == 0.0, 0.0, ws * f[..., k]) for f in (fe, fl, fp) for k in range(d)] + [ws])
    return torch.from_numpy(np.stack(terms))


def grad_sums(x, ls, env, lam, period, s_t, s_s, alpha, p):
    """what pls_kernel_grad_sums computes for PLS_KERNEL_TREND_SEASONAL (4 d + 2 sums), and per output the scale sum_ij |term|"""
    return fsum_rows(pair_terms(x, ls, env, lam, period, s_t, s_s, alpha, p))


def grad_sums_majorant(x, ls, env, lam, period, s_t, s_s, alpha, p):
    """per output the scale S of the reduction test: the fsum of the majorant of its terms"""
    return fsum_rows(pair_terms(x, ls, env, lam, period, s_t, s_s, alpha, p, majorant=True))[0]


def mll_and_grad(x, y, ls, env, lam, period, s_t, s_s, noise, mean, fixed=None):
    """The 4 + 4 d + 1 outputs of pls_gp_mll_grad for PLS_KERNEL_TREND_SEASONAL through LAPACK (Cholesky, cholesky_solve,
    cholesky_inverse) and, per output, its sum-of-magnitudes scale -- exact_gp_truth.lapack_mll_and_grad's evaluation with
    K_y = s_t kappa_t + s_s kappa_s + diag (that function builds K_y from ONE kappa and one outputscale)."""
    x = x if x.dim() == 2 else x[:, None]
    n = x.shape[0]
    diag = torch.full((n,), float(noise), dtype=torch.float64) if fixed is None else fixed.double() + float(noise)
    low = torch.linalg.cholesky(gram(x, ls, env, lam, period, s_t, s_s) + torch.diag(diag))
    r = y.double() - mean
    alpha = torch.cholesky_solve(r[:, None], low)[:, 0]
    p = torch.cholesky_inverse(low)
    p = 0.5 * (p + p.T)
    logs = torch.log(low.diagonal())
    quad = math.fsum((r * alpha).tolist())
    sums, scale = grad_sums(x, ls, env, lam, period, s_t, s_s, alpha, p)
    wdiag = alpha * alpha - p.diagonal()
    out = np.empty(3 + sums.size)
    mag = np.empty_like(out)
    out[0] = -0.5 * quad - math.fsum(logs.tolist()) - 0.5 * n * math.log(2.0 * math.pi)
    mag[0] = 0.5 * abs(quad) + math.fsum(logs.abs().tolist())
    out[1], mag[1] = math.fsum(alpha.tolist()), math.fsum(alpha.abs().tolist())
    out[2], mag[2] = 0.5 * math.fsum(wdiag.tolist()), 0.5 * math.fsum(wdiag.abs().tolist())
    out[3], mag[3] = 0.5 * s_t * sums[0], 0.5 * s_t * scale[0]
    out[4:], mag[4:] = 0.5 * sums[1:], 0.5 * scale[1:]
    return out, mag


def host_evaluate(model):
    """``evaluate`` for train_exact_gp: the model's loss and raw gradient from this module's LAPACK evaluation"""
    out, _ = mll_and_grad(model.x, model.y, model.lengthscale, model.seasonal_lengthscale, model.periodic_lengthscale,
                          model.period_length, model.outputscale, model.seasonal_outputscale, model.noise, model.mean_constant)
    return model.chain_rule(torch.from_numpy(out))


# ---- the fixture's whole-evaluation cases: name -> (n, d, seed) -----------------------------------------------------------
CASES = {"trend-seasonal-n70-d1": (70, 1, 1210701), "trend-seasonal-n65-d3": (65, 3, 1210653),
         "trend-seasonal-n130-d8": (130, 8, 1211308)}


def draw_parameters(g, d):
    """l = (2 + U) sqrt(d), so that the trend is longer than the envelope; m, lambda, p as
    locally_periodic_truth.draw_parameters"""
    ls = (2.0 + _uniform(g, (d,))) * float(np.sqrt(d))
    return (ls,) + seasonal_parameters(g, d)


def case_inputs(name):
    """x ~ N(0, I) (n, d), y = 2 t / (1 + t^2) + 0.3 N(0, 1) with t = sum_k x_k, and draw_parameters: (x, y, l, m, lambda, p)"""
    n, d, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = _normal(g, (n, d))
    t = torch.zeros(n, dtype=torch.float64)
    for k in range(d):
        t = t + x[:, k]
    y = 2.0 * t / (1.0 + t * t) + 0.3 * _normal(g, (n,))
    return (x, y) + draw_parameters(g, d)


def truth(name):
    """the 50-digit outputs (4 + 4 d + 1) of a case as (hi, lo) float64 pairs, after checking that the inputs are the recorded
    ones"""
    return fixture_truth(TRUTH, name, list(case_inputs(name)))


_cpu_cache = {}


def cpu_case(name):
    """(out, scale, e_cpu) of a case: this module's LAPACK evaluation, its scales, and per output its error against the
    50-digit truth relative to the scale -- computed once and shared"""
    if name not in _cpu_cache:
        x, y, ls, env, lam, period = case_inputs(name)
        out, mag = mll_and_grad(x, y, ls, env, lam, period, S_T, S_S, NOISE, MEAN)
        hi, lo = truth(name)
        _cpu_cache[name] = (out, mag, relative_error(out, hi, lo, mag))
    return _cpu_cache[name]
