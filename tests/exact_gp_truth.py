"""The yardstick of the exact-GP tests: closed-form kernels and their lengthscale derivatives, the d + 1 pair sums of
pls_kernel_grad_sums, and the marginal log-likelihood with its gradient through LAPACK -- torch float64 on the CPU, sums
by math.fsum -- together with the case table of tests/golden/exact_gp_truth.npz (50-digit values of the same quantities,
written by tests/golden/make_exact_gp_truth.py).

With e_k = (x_ik - x_jk) / l_k, r^2 = sum_k e_k^2, kappa the kernel without its outputscale s:
    RBF:     kappa = exp(-r^2 / 2),              dK / d log l_k = s exp(-r^2 / 2) e_k^2
    Matern:  kappa = p(t) exp(-t), t = sqrt(2 nu) r,  dK / d log l_k = s q(t) exp(-t) 2 nu e_k^2,
             q = 1/t, 1, (1 + t)/3 for nu = 1/2, 3/2, 5/2
A pair with r = 0 has derivative 0 (also where q = 1/t), a pair whose exponential is 0 contributes 0 everywhere."""
import math
import os

import numpy as np
import torch

from matern_closed_form import matern_torch
from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

RBF, MATERN12, MATERN32, MATERN52 = 0, 2, 3, 4  # pls_kernel_kind
KINDS = (RBF, MATERN12, MATERN32, MATERN52)
NU = {MATERN12: 0.5, MATERN32: 1.5, MATERN52: 2.5}
KIND_NAMES = {RBF: "rbf", MATERN12: "matern12", MATERN32: "matern32", MATERN52: "matern52"}
EPS = 2.0**-52  # machine epsilon of float64 (numpy.finfo(float64).eps)
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_gp_truth.npz")


def _scaled_differences(x, ls):
    x = x if x.dim() == 2 else x[:, None]
    return (x[:, None, :].double() - x[None, :, :].double()) / torch.as_tensor(ls, dtype=torch.float64).reshape(-1)


def kappa(kind, x, ls):
    """kappa(x, x) (n, n): the kernel without its outputscale"""
    if kind == RBF:
        return torch.exp(-0.5 * _scaled_differences(x, ls).square().sum(-1))
    return matern_torch(ls, 1.0, NU[kind])(x, x)


def dk_dlog_lengthscale(kind, x, ls, s):
    """(d, n, n): dK_ij / d log l_k"""
    e = _scaled_differences(x, ls)
    e2 = e.square()
    r2 = e2.sum(-1)
    if kind == RBF:
        ex = torch.exp(-0.5 * r2)
        g = s * ex
    else:
        nu = NU[kind]
        t = torch.sqrt(2.0 * nu * r2)
        ex = torch.exp(-t)
        q = {0.5: torch.where(t > 0, 1.0 / t, torch.zeros_like(t)), 1.5: torch.ones_like(t), 2.5: (1.0 + t) / 3.0}[nu]
        g = s * q * ex * (2.0 * nu)
    dead = (ex == 0.0) | (r2 == 0.0)
    out = g[..., None] * e2
    out = torch.where(dead[..., None], torch.zeros_like(out), out)
    return out.permute(2, 0, 1).contiguous()


def pair_terms(kind, x, ls, s, alpha, p):
    """(d + 1, n, n): the terms of the d + 1 sums, W_ij kappa_ij and W_ij dK_ij / d log l_k, W = alpha alpha^T - P"""
    w = alpha[:, None] * alpha[None, :] - p
    kap = kappa(kind, x, ls)
    head = torch.where(kap == 0.0, torch.zeros_like(kap), w * kap)
    dk = dk_dlog_lengthscale(kind, x, ls, s)
    tail = torch.where(dk == 0.0, torch.zeros_like(dk), w[None] * dk)
    return torch.cat([head[None], tail], dim=0)


def fsum_rows(terms):
    """per leading index: (the exactly rounded sum of the terms, the sum of their magnitudes)"""
    flat = terms.reshape(terms.shape[0], -1).numpy()
    sums = np.array([math.fsum(row) for row in flat])
    scale = np.array([math.fsum(np.abs(row)) for row in flat])
    return sums, scale


def grad_sums(kind, x, ls, s, alpha, p):
    """what pls_kernel_grad_sums computes, and per output the scale sum_ij |term|"""
    return fsum_rows(pair_terms(kind, x, ls, s, alpha, p))


def lapack_mll_and_grad(kap, family_grad_sums, y, s, noise, mean, fixed=None):
    """The one LAPACK evaluation (Cholesky, cholesky_solve, cholesky_inverse) behind every family's ``mll_and_grad``: the
    outputs of pls_gp_mll_grad (of a row of pls_gp_mll_grad_classes when ``fixed`` (n) joins the noise on the diagonal) and,
    per output, its sum-of-magnitudes scale: 1/2 |r^T alpha| + sum |log L_ii| for the value, sum |alpha_i| for d/d mean, and
    S_theta = 1/2 sum_ij |W_ij dK_ij / d theta| for the rest.  The family supplies ``kap`` = kappa(x, x) (n, n) and
    ``family_grad_sums(alpha, p)`` -> (its pair sums, their scales): one output per sum, behind value, d/d mean, d/d noise."""
    n = kap.shape[0]
    diag = torch.full((n,), float(noise), dtype=torch.float64) if fixed is None else fixed.double() + float(noise)
    ky = s * kap + torch.diag(diag)
    low = torch.linalg.cholesky(ky)
    r = y.double() - mean
    alpha = torch.cholesky_solve(r[:, None], low)[:, 0]
    p = torch.cholesky_inverse(low)
    p = 0.5 * (p + p.T)
    logs = torch.log(low.diagonal())
    quad = math.fsum((r * alpha).tolist())
    sums, scale = family_grad_sums(alpha, p)
    wdiag = alpha * alpha - p.diagonal()
    out = np.empty(3 + sums.size)
    mag = np.empty_like(out)
    out[0] = -0.5 * quad - math.fsum(logs.tolist()) - 0.5 * n * math.log(2.0 * math.pi)
    mag[0] = 0.5 * abs(quad) + math.fsum(logs.abs().tolist())
    out[1], mag[1] = math.fsum(alpha.tolist()), math.fsum(alpha.abs().tolist())
    out[2], mag[2] = 0.5 * math.fsum(wdiag.tolist()), 0.5 * math.fsum(wdiag.abs().tolist())
    out[3], mag[3] = 0.5 * s * sums[0], 0.5 * s * scale[0]
    out[4:], mag[4:] = 0.5 * sums[1:], 0.5 * scale[1:]
    return out, mag


def mll_and_grad(kind, x, y, ls, s, noise, mean, fixed=None):
    """The 4 + d outputs of pls_gp_mll_grad for RBF and Matern through LAPACK and their scales (``lapack_mll_and_grad``)"""
    x = x if x.dim() == 2 else x[:, None]
    return lapack_mll_and_grad(kappa(kind, x, ls), lambda alpha, p: grad_sums(kind, x, ls, s, alpha, p), y, s, noise, mean, fixed)


def host_evaluate(model):
    """``evaluate`` for train_exact_gp: the model's loss and raw gradient from this module's LAPACK evaluation"""
    out, _ = mll_and_grad(model.kind, model.x, model.y, model.lengthscale, model.outputscale, model.noise, model.mean_constant)
    return model.chain_rule(torch.from_numpy(out))


# ---- the fixture's cases: name -> (kind, n, d, seed) -------------------------------------------------------------------
OUTPUTSCALE, NOISE, MEAN = 1.3, 0.1, 0.2
CASES = {}
for _n in (1, 2, 65, 130, 260):
    for _d in (1, 3, 8):
        for _kind in (KINDS if _n == 65 else (RBF, MATERN52)):
            CASES[f"{KIND_NAMES[_kind]}-n{_n}-d{_d}"] = (_kind, _n, _d, 500000 + 1000 * _n + 10 * _d + _kind)


def case_inputs(name):
    """x ~ N(0, I) (n, d), y = 2 t / (1 + t^2) + 0.3 N(0, 1) with t = sum_k x_k, lengthscale = (0.5 + U) sqrt(d)"""
    kind, n, d, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = _normal(g, (n, d))
    t = torch.zeros(n, dtype=torch.float64)
    for k in range(d):
        t = t + x[:, k]
    y = 2.0 * t / (1.0 + t * t) + 0.3 * _normal(g, (n,))
    ls = (0.5 + _uniform(g, (d,))) * d**0.5
    return kind, x, y, ls


def truth(name):
    """the 50-digit outputs (4 + d) of a case as (hi, lo) float64 pairs, after checking that the inputs are the recorded ones"""
    return fixture_truth(TRUTH, name, case_inputs(name)[1:])


_cpu_cache = {}


def cpu_case(name):
    """(out, scale, e_cpu) of a case: this module's LAPACK evaluation, its scales, and per output its error against the
    50-digit truth relative to the scale -- computed once and shared"""
    if name not in _cpu_cache:
        kind, x, y, ls = case_inputs(name)
        out, mag = mll_and_grad(kind, x, y, ls, OUTPUTSCALE, NOISE, MEAN)
        hi, lo = truth(name)
        _cpu_cache[name] = (out, mag, relative_error(out, hi, lo, mag))
    return _cpu_cache[name]
