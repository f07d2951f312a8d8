"""The yardstick of the rational-quadratic exact-GP tests, modelled on exact_gp_truth.py: the closed-form kernel and its
derivatives with respect to the lengthscales and the shape alpha, the d + 2 pair sums of pls_kernel_grad_sums, and the
marginal log-likelihood with its 4 + d + 1 derivatives through LAPACK -- torch float64 on the CPU, sums by math.fsum --
together with the tables of tests/golden/rq_truth.npz (50-digit values, written by tests/golden/make_rq_truth.py).

With e_k = (x_ik - x_jk) / l_k, r^2 = sum_k e_k^2, u = r^2 / (2 alpha), kappa = (1 + u)^-alpha the kernel without its
outputscale s:
    dK / d log l_k   = s kappa / (1 + u) e_k^2
    dK / d log alpha = s alpha kappa (u / (1 + u) - log1p(u))
A pair with r = 0 has both derivatives 0; a pair whose kappa is 0 contributes 0 everywhere.  ``shape`` is the kernel's
alpha throughout; ``alpha`` stays the solve's vector K_y^-1 (y - mean), as in exact_gp_truth.py."""
import os

import numpy as np
import torch

from exact_gp_truth import EPS, MEAN, NOISE, OUTPUTSCALE, _scaled_differences, fsum_rows, lapack_mll_and_grad  # noqa: F401
from rq_closed_form import ALPHAS, LN2, rq_factors_numpy
from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

RQ = 6  # pls_kernel_kind
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rq_truth.npz")


def factors(x, ls, shape):
    """(kappa (n, n), g (n, n), ga (n, n), e^2 (n, n, d)) of all pairs of x"""
    e2 = _scaled_differences(x, ls).square()
    kap, g, ga = rq_factors_numpy(e2.sum(-1).numpy(), shape)
    return torch.from_numpy(kap), torch.from_numpy(g), torch.from_numpy(ga), e2


def kappa(x, ls, shape):
    return factors(x, ls, shape)[0]


def pair_terms(x, ls, shape, s, alpha, p):
    """(d + 2, n, n): the terms W_ij kappa_ij, W_ij dK_ij / d log l_k and W_ij dK_ij / d log alpha, W = alpha alpha^T - P"""
    w = alpha[:, None] * alpha[None, :] - p
    kap, g, ga, e2 = factors(x, ls, shape)
    dead = kap == 0.0
    zero = torch.zeros_like(kap)
    head = torch.where(dead, zero, w * kap)
    dk = torch.where((dead | (e2.sum(-1) == 0.0))[..., None], torch.zeros_like(e2), (s * g)[..., None] * e2).permute(2, 0, 1)
    tail = torch.where(dk == 0.0, torch.zeros_like(dk), w[None] * dk)
    last = torch.where(dead | (ga == 0.0), zero, w * (s * ga))
    return torch.cat([head[None], tail, last[None]], dim=0)


def grad_sums(x, ls, shape, s, alpha, p):
    """what pls_kernel_grad_sums computes for PLS_KERNEL_RQ (d + 2 sums), and per output the scale sum_ij |term|"""
    return fsum_rows(pair_terms(x, ls, shape, s, alpha, p))


def mll_and_grad(x, y, ls, shape, s, noise, mean, fixed=None):
    """The 5 + d outputs of pls_gp_mll_grad for PLS_KERNEL_RQ through LAPACK and, per output, its sum-of-magnitudes scale
    (exact_gp_truth.lapack_mll_and_grad with the alpha derivative behind the lengthscale derivatives)"""
    x = x if x.dim() == 2 else x[:, None]
    return lapack_mll_and_grad(kappa(x, ls, shape), lambda alpha, p: grad_sums(x, ls, shape, s, alpha, p), y, s, noise, mean, fixed)


def host_evaluate(model):
    """``evaluate`` for train_exact_gp: the model's loss and raw gradient from this module's LAPACK evaluation"""
    out, _ = mll_and_grad(model.x, model.y, model.lengthscale, model.alpha, model.outputscale, model.noise, model.mean_constant)
    return model.chain_rule(torch.from_numpy(out))


# ---- the fixture's per-pair table ---------------------------------------------------------------------------------------
#: squared scaled distances: 0, the small-u range where the alpha factor cancels, the change of the logarithm's exponent at
#: 1 + u = sqrt 2 for several alpha, ordinary distances, and 1e4 lengthscales away
PAIR_R2 = np.array([0.0, 1e-300, 1e-30, 1e-16, 1e-9, 1e-4, 0.03, 0.0414, 0.0415, 0.5, 0.574, 0.575, 1.0, 2.4852, 2.4853, 7.0,
                    50.0, 828.0, 829.0, 1491.0, 1e4, 1e8, 1e16, 1e300])


def pair_truth():
    """(hi, lo) of shape (len(ALPHAS), 3, len(PAIR_R2)): 50-digit kappa, g and ga per alpha and distance"""
    return fixture_truth(TRUTH, "pairs", [torch.from_numpy(PAIR_R2), torch.tensor(ALPHAS, dtype=torch.float64)])


# ---- the fixture's whole-evaluation cases: name -> (n, d, seed, shape) --------------------------------------------------
CASES = {"rq-n70-d1-a0.05": (70, 1, 610701, 0.05), "rq-n65-d3-aln2": (65, 3, 610653, LN2), "rq-n130-d8-a3": (130, 8, 611308, 3.0)}


def case_inputs(name):
    """x ~ N(0, I) (n, d), y = 2 t / (1 + t^2) + 0.3 N(0, 1) with t = sum_k x_k, lengthscale = (0.5 + U) sqrt(d); the shape"""
    n, d, seed, shape = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = _normal(g, (n, d))
    t = torch.zeros(n, dtype=torch.float64)
    for k in range(d):
        t = t + x[:, k]
    y = 2.0 * t / (1.0 + t * t) + 0.3 * _normal(g, (n,))
    ls = (0.5 + _uniform(g, (d,))) * d**0.5
    return x, y, ls, shape


def truth(name):
    """the 50-digit outputs (5 + d) of a case as (hi, lo) float64 pairs, after checking that the inputs are the recorded ones"""
    return fixture_truth(TRUTH, name, case_inputs(name)[:3])


_cpu_cache = {}


def cpu_case(name):
    """(out, scale, e_cpu) of a case: this module's LAPACK evaluation, its scales, and per output its error against the
    50-digit truth relative to the scale -- computed once and shared"""
    if name not in _cpu_cache:
        x, y, ls, shape = case_inputs(name)
        out, mag = mll_and_grad(x, y, ls, shape, OUTPUTSCALE, NOISE, MEAN)
        hi, lo = truth(name)
        _cpu_cache[name] = (out, mag, relative_error(out, hi, lo, mag))
    return _cpu_cache[name]
