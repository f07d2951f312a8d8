"""The yardstick of the quadrature-likelihood SVGP tests: the minibatch ELBO of the fixed-kernel SVGP with a Bernoulli
(probit) or a Student-t likelihood and its gradient as include/plship.h states them ("SVGP with a quadrature likelihood")
-- numpy float64 on the CPU, every sum by math.fsum, scipy's erfcx / gammaln --, the same ELBO as a differentiable torch
function, the scale S of every output, an SGD loop on autograd of the torch version, and the case table of
tests/golden/svgp_quadrature_truth.npz (50-digit values, written by tests/golden/make_svgp_quadrature_truth.py).

mu_i, w_i, v_i, KL and the layout of the output vector are svgp_truth's.  Per point, with x_k, omega_k the 20 Gauss-Hermite
nodes and weights below (numpy.polynomial.hermite.hermgauss(20) as doubles) and w^_k = omega_k / sqrt(pi) rounded once:
    f_k = mu_i + sqrt(2 v_i) x_k     l_i = sum_k w^_k g(f_k)     g_mu,i = sum_k w^_k g'(f_k)
    g_v,i = (sum_k w^_k g'(f_k) x_k) / sqrt(2 v_i)               [Student-t] d_i = sum_k w^_k dg/ds2(f_k)

The scale S.  svgp_truth's majorant (every input by its magnitude, every subtraction an addition) gives mu_i and v_i their
scales S_mu,i and S_v,i: rounding moves mu_i by about eps S_mu,i and v_i by eps S_v,i, hence f_k by
eps D_k, D_k = S_mu,i + sqrt(2 S_v,i) |x_k|.  To first order that moves g(f_k) by |g'(f_k)| eps D_k, g'(f_k) by |g''| eps D_k
and dg/ds2(f_k) by |d/df dg/ds2(f_k)| eps D_k, so per point
    S_l   = sum_k w^_k (|g(f_k)| + |g'(f_k)| D_k)            S_gmu = sum_k w^_k (|g'(f_k)| + G2 D_k)
    S_gv  = (sum_k w^_k |x_k| (|g'(f_k)| + G2 D_k)) / sqrt(2 v_i) * (1 + S_v,i / (2 v_i))
    S_d   = sum_k w^_k (1 / (2 s2) + (nu + 1) r^2 / (2 s2 d) + |d/df dg/ds2(f_k)| D_k)
with G2 the bound on |g''|: 1 for the probit, (nu + 1) / (nu s^2) for Student-t.  (The last factor of S_gv is the
first-order sensitivity of 1 / sqrt(2 v) to v.)  The assembly into the outputs is svgp_truth's majorant assembly."""
import math
import os

import numpy as np
import torch

import svgp_truth as T
from truth_common import checksum, fixture_truth, relative_error  # noqa: F401

EPS = T.EPS
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svgp_quadrature_truth.npz")
GAUSSIAN, BERNOULLI, STUDENT_T = 0, 1, 2
Q = 20
GH_X = np.array([
    -5.3874808900112328, -4.6036824495507442, -3.9447640401156252, -3.3478545673832163, -2.7888060584281305,
    -2.2549740020892757, -1.7385377121165861, -1.2340762153953231, -0.73747372854539439, -0.24534070830090124,
    0.24534070830090124, 0.73747372854539439, 1.2340762153953231, 1.7385377121165861, 2.2549740020892757,
    2.7888060584281305, 3.3478545673832163, 3.9447640401156252, 4.6036824495507442, 5.3874808900112328])
GH_OMEGA = np.array([
    2.2293936455341447e-13, 4.3993409922731747e-10, 1.0860693707692782e-07, 7.8025564785320599e-06, 0.00022833863601635365,
    0.0032437733422378567, 0.024810520887463643, 0.10901720602002329, 0.28667550536283415, 0.46224366960061009,
    0.46224366960061009, 0.28667550536283415, 0.10901720602002329, 0.024810520887463643, 0.0032437733422378567,
    0.00022833863601635365, 7.8025564785320599e-06, 1.0860693707692782e-07, 4.3993409922731747e-10, 2.2293936455341447e-13])
GH_W = np.array([
    1.2578006724379234e-13, 2.4820623623151755e-10, 6.127490259982928e-08, 4.402121090230851e-06, 0.00012882627996192928,
    0.0018301031310804898, 0.013997837447101022, 0.06150637206397689, 0.16173933398399998, 0.26079306344955483,
    0.26079306344955483, 0.16173933398399998, 0.06150637206397689, 0.013997837447101022, 0.0018301031310804898,
    0.00012882627996192928, 4.402121090230851e-06, 6.127490259982928e-08, 2.4820623623151755e-10, 1.2578006724379234e-13])

#: name -> (likelihood code, degrees of freedom)
LIKELIHOODS = {"bernoulli": (BERNOULLI, 0.0), "student3": (STUDENT_T, 3.0), "student4.5": (STUDENT_T, 4.5)}
INV_SQRT2 = 0.70710678118654752440
SQRT_2_OVER_PI = 0.79788456080286535588
INV_SQRT_2PI = 0.39894228040143267794


def noise_of(lik, rho):
    """the likelihood's noise from the raw value: the Student-t scale^2 has NO 1e-4 floor"""
    return T.softplus(rho) + (T.MIN_NOISE if lik == GAUSSIAN else 0.0)


def log_ndtr(z):
    """log Phi(z), accurate in both tails (numpy float64)"""
    from scipy.special import erfc, erfcx

    z = np.asarray(z, dtype=np.float64)
    neg = z < 0
    zn, zp = np.where(neg, z, 0.0), np.where(neg, 0.0, z)
    return np.where(neg, np.log(0.5 * erfcx(-zn * INV_SQRT2)) - 0.5 * zn * zn, np.log1p(-0.5 * erfc(zp * INV_SQRT2)))


def hazard(z):
    """phi(z) / Phi(z)"""
    from scipy.special import erfc, erfcx

    z = np.asarray(z, dtype=np.float64)
    neg = z < 0
    zn, zp = np.where(neg, z, 0.0), np.where(neg, 0.0, z)
    return np.where(neg, SQRT_2_OVER_PI / erfcx(-zn * INV_SQRT2),
                    INV_SQRT_2PI * np.exp(-0.5 * zp * zp) / (1.0 - 0.5 * erfc(zp * INV_SQRT2)))


def node_terms(lik, nu, y, f, sig2):
    """(g, g', dg/ds2, G2 = the bound on |g''|, |d/df dg/ds2|) at the nodes f (..., Q) of the points y (..., 1)"""
    if lik == BERNOULLI:
        s = 2.0 * y - 1.0
        z = s * f
        return log_ndtr(z), s * hazard(z), np.zeros_like(f), 1.0, np.zeros_like(f)
    from scipy.special import gammaln

    r = y - f
    a = nu * sig2
    d = a + r * r
    g = gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu) - 0.5 * math.log(nu * math.pi * sig2) - 0.5 * (nu + 1.0) * np.log1p(r * r / a)
    gp = (nu + 1.0) * r / d
    gs = -0.5 / sig2 + (nu + 1.0) * r * r / (2.0 * sig2 * d)
    gsf = (nu + 1.0) * np.abs(r) * a / (sig2 * d * d)  # |d/df of (nu + 1) r^2 / (2 s2 d)|
    return g, gp, gs, (nu + 1.0) / a, gsf


def evaluate(lik, nu, At, q, y, mean, Ls, c, rho, idx, n, scale=False):
    """The output vector of one minibatch (numpy float64, fsum sums); ``scale=True``: its scale vector S instead."""
    At, q, y, mean, Ls = (np.asarray(t, dtype=np.float64) for t in (At, q, y, mean, Ls))
    idx = np.arange(n) if idx is None else np.asarray(idx)
    a, qb, yb = At[idx], q[idx], y[idx]
    b, m = a.shape
    low = np.tril(Ls)
    sig2 = noise_of(lik, rho)
    mu = c + T._fsum_last(a * mean[None, :])
    w = T._fsum_last(a[:, None, :] * low.T[None, :, :])
    v = qb + T._fsum_last(w * w)
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(2.0 * v)
        f = mu[:, None] + sq[:, None] * GH_X[None, :]
        g, gp, gs, g2, gsf = node_terms(lik, nu, yb[:, None], f, sig2)
        if not scale:
            ell = T._fsum_last(GH_W * g)
            gmu = T._fsum_last(GH_W * gp)
            gv = T._fsum_last(GH_W * GH_X * gp) / sq
            ds = T._fsum_last(GH_W * gs)
            aa, ww, mm, ll, sgn = a, w, mean, low, 1.0
        else:
            aa, mm, ll, sgn = np.abs(a), np.abs(mean), np.abs(low), -1.0
            s_mu = abs(c) + T._fsum_last(aa * mm[None, :])
            ww = T._fsum_last(aa[:, None, :] * ll.T[None, :, :])
            s_v = np.abs(qb) + T._fsum_last(ww * ww)
            dk = s_mu[:, None] + np.sqrt(2.0 * s_v)[:, None] * np.abs(GH_X)[None, :]
            ell = T._fsum_last(GH_W * (np.abs(g) + np.abs(gp) * dk))
            gmu = T._fsum_last(GH_W * (np.abs(gp) + g2 * dk))
            gv = T._fsum_last(GH_W * np.abs(GH_X) * (np.abs(gp) + g2 * dk)) / sq * (1.0 + s_v / (2.0 * v))
            if lik == STUDENT_T:
                r2 = (yb[:, None] - f) ** 2
                ds = T._fsum_last(GH_W * (0.5 / sig2 + (nu + 1.0) * r2 / (2.0 * sig2 * (nu * sig2 + r2)) + gsf * dk))
            else:
                ds = np.zeros(b)
    diag = np.diagonal(ll)
    logd = np.log(np.abs(diag))
    tri = T.lower_entries(ll)
    if not scale:
        kl = 0.5 * (math.fsum(tri * tri) + math.fsum(mm * mm) - m - 2.0 * math.fsum(logd))
    else:
        kl = 0.5 * (math.fsum(tri * tri) + math.fsum(mm * mm) + m + 2.0 * math.fsum(np.abs(logd)))
    ell_mean = math.fsum(ell) / b
    out = np.empty(5 + m + m * (m + 1) // 2)
    out[0] = ell_mean - sgn * kl / n
    out[1] = math.fsum(gmu) / b
    out[2] = T.sigmoid(rho) * math.fsum(ds) / b if lik == STUDENT_T else 0.0
    out[3], out[4] = ell_mean, kl
    out[5:5 + m] = T._fsum_last((gmu[:, None] * aa).T) / b - sgn * mm / n
    k_idx, l_idx = np.tril_indices(m)
    terms = gv[:, None] * aa[:, k_idx] * ww[:, l_idx]
    pen = ll[k_idx, l_idx].copy()
    with np.errstate(divide="ignore"):
        inv = 1.0 / diag
    pen[k_idx == l_idx] = (diag - inv) if not scale else (diag + np.abs(inv))
    out[5 + m:] = 2.0 * T._fsum_last(terms.T) / b - sgn * pen / n
    return out


# ---- the same ELBO in torch, differentiable in mean, Ls, c, rho -----------------------------------------------------------
def _log_ndtr_torch(z):
    neg = z < 0
    zn, zp = torch.where(neg, z, torch.zeros_like(z)), torch.where(neg, torch.zeros_like(z), z)
    return torch.where(neg, torch.log(0.5 * torch.special.erfcx(-zn * INV_SQRT2)) - 0.5 * zn * zn,
                       torch.log1p(-0.5 * torch.erfc(zp * INV_SQRT2)))


_node_cache = {}


def _nodes(device):
    if device not in _node_cache:
        _node_cache[device] = (torch.from_numpy(GH_X).to(device), torch.from_numpy(GH_W).to(device))
    return _node_cache[device]


def elbo_torch(lik, nu, At, q, y, mean, Ls, c, rho, idx, n):
    a = At if idx is None else At[idx]
    qb = q if idx is None else q[idx]
    yb = y if idx is None else y[idx]
    low = torch.tril(Ls)
    mu = c + a @ mean
    w = a @ low
    v = qb + (w * w).sum(dim=1)
    x, wq = _nodes(a.device)
    f = mu[:, None] + torch.sqrt(2.0 * v)[:, None] * x[None, :]
    if lik == BERNOULLI:
        g = _log_ndtr_torch((2.0 * yb[:, None] - 1.0) * f)
    else:
        sig2 = torch.nn.functional.softplus(rho, threshold=1e9)
        r = yb[:, None] - f
        g = (math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * torch.log(nu * math.pi * sig2)
             - 0.5 * (nu + 1.0) * torch.log1p(r * r / (nu * sig2)))
    ell = (g * wq).sum(dim=1)
    kl = 0.5 * ((low * low).sum() + (mean * mean).sum() - mean.shape[0] - 2.0 * torch.log(low.diagonal().abs()).sum())
    return ell.mean() - kl / n


def gradients_autograd(lik, nu, At, q, y, mean, Ls, c, rho, idx, n):
    """(ELBO, d/dm, d/dL_s (lower), d/dc, d/drho) by autograd of elbo_torch (detached tensors; d/drho 0 for Bernoulli)"""
    mean, Ls, c, rho = (t.detach().clone().requires_grad_(True) for t in (mean, Ls, c, rho))
    elbo = elbo_torch(lik, nu, At, q, y, mean, Ls, c, rho, idx, n)
    g_m, g_l, g_c, g_rho = torch.autograd.grad(elbo, (mean, Ls, c, rho), allow_unused=True)
    return elbo.detach(), g_m, torch.tril(g_l), g_c, torch.zeros_like(rho) if g_rho is None else g_rho


def sgd_loop(lik, nu, At, q, y, mean, Ls, c, rho, batches_per_epoch, lr, train_mean=True, train_noise=True, perturb=0.0):
    """svgp_truth.sgd_loop with this ELBO; a Bernoulli likelihood never moves rho.  Returns (losses, mean, Ls, c, rho)."""
    n = At.shape[0]
    mean, Ls = mean.clone(), torch.tril(Ls.clone())
    c, rho = torch.tensor(float(c), dtype=torch.float64), torch.tensor(float(rho), dtype=torch.float64)

    def jolt(t):
        if not perturb:
            return t
        sign = 1.0 - 2.0 * (torch.arange(t.numel(), dtype=torch.float64) % 2).reshape(t.shape)
        return t * (1.0 + perturb * sign)

    losses = []
    for batches in batches_per_epoch:
        for idx in batches:
            _, g_m, g_l, g_c, g_rho = gradients_autograd(lik, nu, At, q, y, mean, Ls, c, rho, idx, n)
            mean = mean - lr * (-jolt(g_m))
            Ls = Ls - lr * (-jolt(g_l))
            if train_mean:
                c = c - lr * (-jolt(g_c))
            if train_noise and lik != BERNOULLI:
                rho = rho - lr * (-jolt(g_rho))
        with torch.no_grad():
            losses.append(-float(elbo_torch(lik, nu, At, q, y, mean, Ls, c, rho, None, n)))
    return losses, mean, Ls, float(c), float(rho)


# ---- cases: svgp_truth's grid and generator; Bernoulli labels are y > 0 -----------------------------------------------------
CASES = T.CASES
N_FIXTURE = T.N_FIXTURE


def with_targets(lik_name, inp):
    """the inputs of svgp_truth.make_inputs with the targets of the likelihood: labels y > 0 for Bernoulli"""
    if LIKELIHOODS[lik_name][0] == BERNOULLI:
        inp = dict(inp, y=(inp["y"] > 0).double())
    return inp


def case_inputs(lik_name, name):
    return with_targets(lik_name, T.case_inputs(name))


def evaluate_inputs(lik_name, inp, scale=False):
    lik, nu = LIKELIHOODS[lik_name]
    return evaluate(lik, nu, inp["At"].numpy(), inp["q"].numpy(), inp["y"].numpy(), inp["mean"].numpy(), inp["Ls"].numpy(),
                    inp["c"], inp["rho"], None if inp["idx"] is None else inp["idx"].numpy(), inp["n"], scale)


def truth(lik_name, name):
    """the 50-digit output vector of a fixture case as (hi, lo), after checking that the inputs are the recorded ones"""
    return fixture_truth(TRUTH, f"{lik_name}/{name}", T.hashed(case_inputs(lik_name, name)))


_cpu_cache = {}


def cpu_case(lik_name, name):
    """(inputs, fsum output vector, scale vector) of a fixture case, computed once and shared"""
    key = (lik_name, name)
    if key not in _cpu_cache:
        inp = case_inputs(lik_name, name)
        _cpu_cache[key] = (inp, evaluate_inputs(lik_name, inp), evaluate_inputs(lik_name, inp, scale=True))
    return _cpu_cache[key]


_allowance = []


def epilogue_allowance():
    """(the fsum helper's worst error against the 50-digit fixture in units of eps S over every case and likelihood, and
    c = 16 x that, floor 16): the tests allow (M + B + 16 + c) eps S per output.  The margin of 16 covers a device erfcx /
    log1p / log a few ulp off where scipy's are about one."""
    if not _allowance:
        worst = 0.0
        for lik_name in LIKELIHOODS:
            for name in CASES:
                _, out, scale = cpu_case(lik_name, name)
                hi, lo = truth(lik_name, name)
                worst = max(worst, float(relative_error(out, hi, lo, scale).max()) / EPS)
        _allowance.append((worst, max(16.0 * worst, 16.0)))
    return _allowance[0]


def bar(m, b):
    """the tests' bound per output, in units of its scale S"""
    return (m + b + 16 + epilogue_allowance()[1]) * EPS
