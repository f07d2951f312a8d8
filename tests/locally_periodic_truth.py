"""The yardstick of the locally periodic exact-GP tests, modelled on periodic_truth.py: the closed-form kernel and its
derivatives with respect to the envelope lengthscales, the periodic lengthscales and the period lengths, the 3 d + 1 pair sums
of pls_kernel_grad_sums, and the marginal log-likelihood with its 4 + 3 d derivatives through LAPACK -- float64 on the CPU,
sums by math.fsum -- together with the tables of tests/golden/locally_periodic_truth.npz (50-digit values, written by
tests/golden/make_locally_periodic_truth.py).

With delta_k = x_ik - x_jk, e_k = delta_k / p_k and kappa = exp(-(1/2 sum_k (delta_k / l_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k))
the kernel without its outputscale s:
    dK / d log l_k      = s kappa (delta_k / l_k)^2
    dK / d log lambda_k = s kappa (2 / lambda_k) sin^2(pi e_k)
    dK / d log p_k      = s kappa (2 / lambda_k) pi e_k sin(2 pi e_k)
A pair at distance 0 has all three derivatives 0; a pair whose kappa is 0 contributes 0 everywhere."""
import os

import numpy as np
import torch

from exact_gp_truth import EPS, MEAN, NOISE, OUTPUTSCALE, fsum_rows, lapack_mll_and_grad  # noqa: F401
from locally_periodic_closed_form import locally_periodic_factors_numpy, sensitivity
from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

LOCALLY_PERIODIC = 10  # pls_kernel_kind
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "locally_periodic_truth.npz")


def _np(v):
    return (v.detach().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64))


def factors(x, ls, lam, period):
    """(kappa (n, n), fe, fl, fp, e (n, n, d) each, delta (n, n, d)) of all pairs of x, numpy"""
    x = _np(x)
    x = x if x.ndim == 2 else x[:, None]
    delta = x[:, None, :] - x[None, :, :]
    return locally_periodic_factors_numpy(delta, _np(ls), _np(lam), _np(period)) + (delta,)


def kappa(x, ls, lam, period):
    return torch.from_numpy(factors(x, ls, lam, period)[0])


def pair_terms(x, ls, lam, period, s, alpha, p, majorant=False):
    """(3 d + 1, n, n): the terms W_ij kappa_ij, W_ij dK_ij / d log l_k, W_ij dK_ij / d log lambda_k and W_ij dK_ij / d log p_k,
    W = alpha alpha^T - P.  ``majorant``: instead of each term what bounds its first-order error budget -- |W| kappa,
    |W| s kappa fe_k, |W| s kappa fl_k and |W| s kappa (2 / lambda_k) pi |e_k| (the period term with |sin(2 pi e)| replaced by 1),
    each times the pair's sensitivity c_ij = 1 + r_ij^2 + sum_k (2 pi / lambda_k) |e_k| (locally_periodic_closed_form.sensitivity)."""
    w = _np(alpha)[:, None] * _np(alpha)[None, :] - _np(p)
    kap, fe, fl, fp, e, delta = factors(x, ls, lam, period)
    lam = _np(lam).reshape(-1)
    d = lam.size
    if majorant:
        c = sensitivity(delta, e, _np(ls), lam)
        aw = np.abs(w) * kap * c
        per = (2.0 / lam) * np.pi * np.abs(e)
        terms = ([aw] + [aw * s * fe[..., k] for k in range(d)] + [aw * s * fl[..., k] for k in range(d)] +
                 [aw * s * per[..., k] for k in range(d)])
    else:
        wk = np.where(kap == 0.0, 0.0, w * kap)
        with np.errstate(invalid="ignore", over="ignore"):  # (a dead pair's fe may be inf: its terms are selected to 0)
            terms = [wk] + [np.where(kap == 0.0, 0.0, wk * (s * f[..., k])) for f in (fe, fl, fp) for k in range(d)]
    return torch.from_numpy(np.stack(terms))


def grad_sums(x, ls, lam, period, s, alpha, p):
    """what pls_kernel_grad_sums computes for PLS_KERNEL_LOCALLY_PERIODIC (3 d + 1 sums), and per output the scale sum_ij |term|"""
    return fsum_rows(pair_terms(x, ls, lam, period, s, alpha, p))


def grad_sums_majorant(x, ls, lam, period, s, alpha, p):
    """per output the scale S of the reduction test: the fsum of the majorant of its terms"""
    return fsum_rows(pair_terms(x, ls, lam, period, s, alpha, p, majorant=True))[0]


def mll_and_grad(x, y, ls, lam, period, s, noise, mean, fixed=None):
    """The 4 + 3 d outputs of pls_gp_mll_grad for PLS_KERNEL_LOCALLY_PERIODIC through LAPACK and, per output, its
    sum-of-magnitudes scale (exact_gp_truth.lapack_mll_and_grad with the shape derivatives behind the lengthscale derivatives)"""
    x = x if x.dim() == 2 else x[:, None]
    return lapack_mll_and_grad(kappa(x, ls, lam, period), lambda alpha, p: grad_sums(x, ls, lam, period, s, alpha, p), y, s, noise,
                               mean, fixed)


def host_evaluate(model):
    """``evaluate`` for train_exact_gp: the model's loss and raw gradient from this module's LAPACK evaluation"""
    out, _ = mll_and_grad(model.x, model.y, model.lengthscale, model.periodic_lengthscale, model.period_length, model.outputscale,
                          model.noise, model.mean_constant)
    return model.chain_rule(torch.from_numpy(out))


# ---- the fixture's per-pair table (d = 1) -------------------------------------------------------------------------------
#: e = delta / p: 0, the small-argument range, the swap of sine and cosine at 1/4, the rounding boundary at 1/2 and its two
#: neighbours, a whole period (the envelope keeps kappa below 1 there), ordinary values, and one pair that the envelope kills
PAIR_E = np.array([0.0, 1e-300, 1e-16, 1e-9, 0.25, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 1.0, 0.1, 0.3, 0.77, 1.4,
                   2.6, -0.37, 7.125, 33.3, 1000.25])
PAIR_PERIODS = (1.0, 0.7, 2.0**-3)
PAIR_PERIODIC_LENGTHSCALE = 0.8
PAIR_LENGTHSCALE = 3.0


def pair_deltas():
    """(len(PAIR_PERIODS), len(PAIR_E)): the differences fl(e p) the table is evaluated at"""
    return np.stack([PAIR_E * p for p in PAIR_PERIODS])


def pair_parameters():
    return torch.tensor(PAIR_PERIODS + (PAIR_PERIODIC_LENGTHSCALE, PAIR_LENGTHSCALE), dtype=torch.float64)


def pair_truth():
    """(hi, lo) of shape (len(PAIR_PERIODS), 4, len(PAIR_E)): 50-digit kappa, fe, fl and fp per period and difference"""
    return fixture_truth(TRUTH, "pairs", [torch.from_numpy(pair_deltas()), pair_parameters()])


# ---- the fixture's whole-evaluation cases: name -> (n, d, seed) -----------------------------------------------------------
CASES = {"locally-periodic-n70-d1": (70, 1, 1010701), "locally-periodic-n65-d3": (65, 3, 1010653),
         "locally-periodic-n130-d8": (130, 8, 1011308)}


def draw_parameters(g, d):
    """l = (1 + U) sqrt(d), lambda = (0.5 + U) d, p = 0.5 + 2.5 U: with x ~ N(0, I) most entries of K stay of the size of s"""
    ls = (1.0 + _uniform(g, (d,))) * float(np.sqrt(d))
    lam = (0.5 + _uniform(g, (d,))) * d
    period = 0.5 + 2.5 * _uniform(g, (d,))
    return ls, lam, period


def case_inputs(name):
    """x ~ N(0, I) (n, d), y = 2 t / (1 + t^2) + 0.3 N(0, 1) with t = sum_k x_k, and draw_parameters"""
    n, d, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = _normal(g, (n, d))
    t = torch.zeros(n, dtype=torch.float64)
    for k in range(d):
        t = t + x[:, k]
    y = 2.0 * t / (1.0 + t * t) + 0.3 * _normal(g, (n,))
    return (x, y) + draw_parameters(g, d)


def truth(name):
    """the 50-digit outputs (4 + 3 d) of a case as (hi, lo) float64 pairs, after checking that the inputs are the recorded ones"""
    return fixture_truth(TRUTH, name, list(case_inputs(name)))


_cpu_cache = {}


def cpu_case(name):
    """(out, scale, e_cpu) of a case: this module's LAPACK evaluation, its scales, and per output its error against the
    50-digit truth relative to the scale -- computed once and shared"""
    if name not in _cpu_cache:
        x, y, ls, lam, period = case_inputs(name)
        out, mag = mll_and_grad(x, y, ls, lam, period, OUTPUTSCALE, NOISE, MEAN)
        hi, lo = truth(name)
        _cpu_cache[name] = (out, mag, relative_error(out, hi, lo, mag))
    return _cpu_cache[name]
