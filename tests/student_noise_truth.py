"""The yardstick of the Student-t noise tests (helpers only, no tests): the terms of the fused predictive mean
(pls_kernel_mean) per test point, and the zero-location Student-t log-likelihood with its derivatives in (log nu, log s) --
float64 on the CPU, every sum by math.fsum, every sum with the sum of the magnitudes of its terms beside it -- together
with the case table of tests/golden/student_noise_truth.npz (50-digit gradient and Hessian, written by
tests/golden/make_student_noise_truth.py).

With u_i = r_i^2 / (nu s^2), A = sum log1p(u), B = sum u / (1 + u), C = sum u / (1 + u)^2, a = log nu, b = log s and
h(nu) = lgamma((nu + 1)/2) - lgamma(nu/2) - log(nu pi)/2:
    ll     = n h - n b - (nu + 1)/2 A
    ll_a   = n nu h' - nu/2 A + (nu + 1)/2 B            h'  = psi((nu + 1)/2)/2 - psi(nu/2)/2 - 1/(2 nu)
    ll_b   = -n + (nu + 1) B
    ll_aa  = n nu h' + n nu^2 h'' - nu/2 A + nu B - (nu + 1)/2 C      h'' = psi'((nu + 1)/2)/4 - psi'(nu/2)/4 + 1/(2 nu^2)
    ll_ab  = nu B - (nu + 1) C
    ll_bb  = -2 (nu + 1) C
The "terms" of a quantity are the products it is evaluated from: per point the pieces of A, B and C with their factors,
and n times each piece of h, h', h'' (the two psi values and the rational part separately)."""
import math
import os

import numpy as np
import torch

from exact_gp_truth import EPS, KIND_NAMES, KINDS, MATERN12, MATERN32, MATERN52, NU, RBF  # noqa: F401
from matern_closed_form import matern_torch
from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "student_noise_truth.npz")


# ---- the fused predictive mean ------------------------------------------------------------------------------------------
def cross_kappa(kind, xt, x, ls):
    """kappa(xt, x) (t, n): the kernel without its outputscale; an entry whose exponential is 0 is exactly 0"""
    xt = xt if xt.dim() == 2 else xt[:, None]
    x = x if x.dim() == 2 else x[:, None]
    if kind == RBF:
        e = (xt[:, None, :].double() - x[None, :, :].double()) / torch.as_tensor(ls, dtype=torch.float64).reshape(-1)
        return torch.exp(-0.5 * e.square().sum(-1))
    return matern_torch(ls, 1.0, NU[kind])(xt, x)


def kernel_mean(kind, x, ls, s, mean, alpha, xt):
    """what pls_kernel_mean computes: per test point (the exactly rounded sum of mean and the terms s kappa_ij alpha_j,
    S_i = |mean| + s sum_j |kappa_ij alpha_j|)"""
    terms = (float(s) * (cross_kappa(kind, xt, x, ls) * alpha.double()[None, :])).numpy()
    want = np.array([math.fsum([float(mean)] + row.tolist()) for row in terms])
    scale = np.array([abs(float(mean)) + math.fsum(np.abs(row).tolist()) for row in terms])
    return want, scale


# ---- the Student-t likelihood -------------------------------------------------------------------------------------------
def _u(r, nu, s):
    r = np.asarray(torch.as_tensor(r).detach().cpu().reshape(-1).numpy(), dtype=np.float64)
    return r * r / (nu * s * s)


def student_sums(r, nu, s):
    """(A, B, C) by math.fsum: the ``evaluate`` of fit_student_t on the CPU"""
    u = _u(r, nu, s)
    return math.fsum(np.log1p(u).tolist()), math.fsum((u / (1.0 + u)).tolist()), math.fsum((u / ((1.0 + u) * (1.0 + u))).tolist())


def trigamma(x: float) -> float:
    """psi'(x) for x > 0: the recurrence psi'(x) = psi'(x + 1) + 1/x^2 up to x >= 15, then the asymptotic series through
    x^-15 (truncation below 1e-18 there); torch's polygamma(1, .) is good to 1e-10 only"""
    total = 0.0
    while x < 15.0:
        total += 1.0 / (x * x)
        x += 1.0
    w = 1.0 / (x * x)
    series = w * (1.0 / 6 + w * (-1.0 / 30 + w * (1.0 / 42 + w * (-1.0 / 30 + w * (5.0 / 66 + w * (-691.0 / 2730 + w * 7.0 / 6))))))
    return total + (1.0 / x + 0.5 * w + series / x)


def _h_pieces(nu):
    """(pieces of h, of h', of h''): each a list of signed numbers whose sum is the quantity"""
    half = torch.tensor([0.5 * (nu + 1.0), 0.5 * nu], dtype=torch.float64)
    psi, tri = torch.special.digamma(half).tolist(), [trigamma(0.5 * (nu + 1.0)), trigamma(0.5 * nu)]
    h = [math.lgamma(0.5 * (nu + 1.0)), -math.lgamma(0.5 * nu), -0.5 * math.log(nu * math.pi)]
    h1 = [0.5 * psi[0], -0.5 * psi[1], -0.5 / nu]
    h2 = [0.25 * tri[0], -0.25 * tri[1], 0.5 / (nu * nu)]
    return h, h1, h2


def _total(pieces):
    """(fsum of the pieces, fsum of their magnitudes)"""
    return math.fsum(pieces), math.fsum(abs(p) for p in pieces)


def student_derivatives(r, nu, s):
    """dict of (value, sum of magnitudes) pairs of the LOG-likelihood of the residuals at (nu, s): "ll", the gradient "a",
    "b" and the Hessian "aa", "ab", "bb" in (a, b) = (log nu, log s)"""
    u = _u(r, nu, s)
    n = u.size
    la, lb, lc = np.log1p(u).tolist(), (u / (1.0 + u)).tolist(), (u / ((1.0 + u) * (1.0 + u))).tolist()
    h, h1, h2 = _h_pieces(nu)
    logs = math.log(s)
    out = {}
    out["ll"] = _total([n * p for p in h] + [-n * logs] + [-0.5 * (nu + 1.0) * v for v in la])
    out["a"] = _total([n * nu * p for p in h1] + [-0.5 * nu * v for v in la] + [0.5 * (nu + 1.0) * v for v in lb])
    out["b"] = _total([-float(n)] + [(nu + 1.0) * v for v in lb])
    out["aa"] = _total([n * nu * p for p in h1] + [n * nu * nu * p for p in h2] + [-0.5 * nu * v for v in la]
                       + [nu * v for v in lb] + [-0.5 * (nu + 1.0) * v for v in lc])
    out["ab"] = _total([nu * v for v in lb] + [-(nu + 1.0) * v for v in lc])
    out["bb"] = _total([-2.0 * (nu + 1.0) * v for v in lc])
    return out


def negative_log_likelihood(r, nu, s):
    """(nll, sum of the magnitudes of its terms)"""
    ll, mag = student_derivatives(r, nu, s)["ll"]
    return -ll, mag


def stationarity(r, nu, s):
    """per gradient component k in (a, b): (|g_k|, the bar 2 (n + 64) eps S_k) -- the bar is the rounding error of
    evaluating the gradient from its terms (a sum of n + O(1) terms, each with a few roundings of its own); an optimiser
    cannot certify less"""
    n = torch.as_tensor(r).numel()
    d = student_derivatives(r, nu, s)
    return [(abs(d[k][0]), 2.0 * (n + 64) * EPS * d[k][1]) for k in ("a", "b")]


# ---- the fixture's cases: name -> (n, nu, s, seed) ------------------------------------------------------------------------
CASES = {"n50-nu3": (50, 3.0, 0.5, 910050), "n257-nu0.7": (257, 0.7, 1.3, 910257), "n1000-nu40": (1000, 40.0, 0.25, 911000)}
OUTPUTS = ("a", "b", "aa", "ab", "bb")


def case_inputs(name):
    """residuals with heavier tails than a normal from integer draws: r = 0.4 z / sqrt(0.05 + u), z ~ N(0, 1), u ~ U(0, 1)"""
    n, _, _, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    return 0.4 * _normal(g, (n,)) / torch.sqrt(0.05 + _uniform(g, (n,)))


def truth(name):
    """the 50-digit (ll_a, ll_b, ll_aa, ll_ab, ll_bb) of a case as (hi, lo) float64 pairs"""
    return fixture_truth(TRUTH, name, [case_inputs(name)])


def student_t_samples(n, nu, s, seed=0):
    """n zero-location Student-t residuals with nu degrees of freedom and scale s, a fixed seed"""
    rng = np.random.RandomState(1000 * seed + n)
    return torch.from_numpy(s * rng.standard_t(nu, size=n))
