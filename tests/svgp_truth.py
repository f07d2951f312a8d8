"""The yardstick of the SVGP tests: the minibatch ELBO of the fixed-kernel SVGP (Gaussian likelihood) and its gradient as
include/plship.h states them -- torch / numpy float64 on the CPU, every sum by math.fsum -- the same ELBO as a
differentiable torch function, the MAJORANT evaluation that gives every output its scale, a plain SGD loop, the
closed-form full-batch optimum, and the case table of tests/golden/svgp_truth.npz (50-digit values, written by
tests/golden/make_svgp_truth.py).

With a_i the rows of At, the state m, L_s (lower), c, rho and sigma^2 = softplus(rho) + 1e-4:
    mu_i = c + a_i . m     w_i = L_s^T a_i     v_i = q_i + |w_i|^2
    l_i  = -1/2 log 2 pi - 1/2 log sigma^2 - ((y_i - mu_i)^2 + v_i) / (2 sigma^2)
    KL   = 1/2 (|tril L_s|_F^2 + |m|^2 - M - 2 sum_p log |L_s,pp|)          ELBO = (1/B) sum_i l_i - KL / N
An output vector is laid out as  [ELBO, d/dc, d/drho, (1/B) sum l_i, KL,  d/dm (M),  d/dL_s lower triangle row by row].

The majorant: the same formulas with every input replaced by its magnitude, every subtraction by an addition and
(y - mu)^2 by (|y| + mu_maj)^2: per output the sum of the magnitudes of everything that enters it, S.  Any summation
order over at most M + B float64 products errs by at most about (M + B) eps S; the tests allow (M + B + 16) eps S."""
import math
import os

import numpy as np
import torch

from truth_common import _normal, _uniform, checksum, fixture_truth, relative_error  # noqa: F401

EPS = 2.0**-52
MIN_NOISE = 1e-4
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svgp_truth.npz")
N_FIXTURE = 200


def softplus(x):
    return max(x, 0.0) + math.log1p(math.exp(-abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


def bar(m, b):
    """the tests' bound per output, in units of its scale S"""
    return (m + b + 16) * EPS


def _fsum_last(a):
    """math.fsum over the last axis"""
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(-1, a.shape[-1])
    return np.array([math.fsum(row) for row in flat]).reshape(a.shape[:-1])


def lower_entries(mat):
    """the lower triangle (diagonal included) row by row"""
    mat = np.asarray(mat)
    k, l = np.tril_indices(mat.shape[0])
    return mat[k, l]


def evaluate(At, q, y, mean, Ls, c, rho, idx, n, majorant=False):
    """The output vector of one minibatch (numpy float64, fsum sums); ``majorant=True``: its scale vector S instead.
    At (n, M), q, y (n), mean (M), Ls (M, M; only the lower triangle is read), idx (B) int64 or None."""
    At, q, y, mean, Ls = (np.asarray(t, dtype=np.float64) for t in (At, q, y, mean, Ls))
    idx = np.arange(n) if idx is None else np.asarray(idx)
    a, qb, yb = At[idx], q[idx], y[idx]
    b, m = a.shape
    low = np.tril(Ls)
    sgn = 1.0
    if majorant:
        a, qb, yb, mean, low, c, sgn = np.abs(a), np.abs(qb), np.abs(yb), np.abs(mean), np.abs(low), abs(c), -1.0
    sig2 = softplus(rho) + MIN_NOISE
    mu = c + _fsum_last(a * mean[None, :])
    w = _fsum_last(a[:, None, :] * low.T[None, :, :])  # w[i, l] = sum_p a[i, p] L[p, l]
    v = qb + _fsum_last(w * w)
    r = yb - sgn * mu  # (majorant: |y| + mu)
    e = r * r + v
    h = 0.5 / sig2
    logs = 0.5 * math.log(sig2)
    ell = (-HALF_LOG_2PI - logs - e * h) if not majorant else (HALF_LOG_2PI + abs(logs) + e * h)
    gmu = r / sig2
    gv = -h if not majorant else h
    ds = (-h + e * h / sig2) if not majorant else (h + e * h / sig2)
    diag = np.diagonal(low)
    logd = np.log(np.abs(diag))
    tri = lower_entries(low)
    if not majorant:
        kl = 0.5 * (math.fsum(tri * tri) + math.fsum(mean * mean) - m - 2.0 * math.fsum(logd))
    else:
        kl = 0.5 * (math.fsum(tri * tri) + math.fsum(mean * mean) + m + 2.0 * math.fsum(np.abs(logd)))
    ell_mean = math.fsum(ell) / b
    out = np.empty(5 + m + m * (m + 1) // 2)
    out[0] = ell_mean - sgn * kl / n
    out[1] = math.fsum(gmu) / b
    out[2] = sigmoid(rho) * math.fsum(ds) / b
    out[3], out[4] = ell_mean, kl
    out[5:5 + m] = _fsum_last((gmu[:, None] * a).T) / b - sgn * mean / n
    # sum_i g_v a_i[k] w_i[l]
    k_idx, l_idx = np.tril_indices(m)
    terms = gv * a[:, k_idx] * w[:, l_idx]  # (B, entries)
    pen = low[k_idx, l_idx].copy()
    with np.errstate(divide="ignore"):
        inv = 1.0 / diag
    pen[k_idx == l_idx] = (diag - sgn * inv) if not majorant else (diag + np.abs(inv))
    out[5 + m:] = 2.0 * _fsum_last(terms.T) / b - sgn * pen / n
    return out


def elbo_torch(At, q, y, mean, Ls, c, rho, idx, n):
    """the same ELBO, differentiable in mean, Ls, c, rho (torch float64 tensors on any device)"""
    a = At if idx is None else At[idx]
    qb = q if idx is None else q[idx]
    yb = y if idx is None else y[idx]
    low = torch.tril(Ls)
    sig2 = torch.nn.functional.softplus(rho, threshold=1e9) + MIN_NOISE
    mu = c + a @ mean
    w = a @ low
    v = qb + (w * w).sum(dim=1)
    ell = -HALF_LOG_2PI - 0.5 * torch.log(sig2) - ((yb - mu) ** 2 + v) / (2.0 * sig2)
    kl = 0.5 * ((low * low).sum() + (mean * mean).sum() - mean.shape[0] - 2.0 * torch.log(low.diagonal().abs()).sum())
    return ell.mean() - kl / n


def gradients_torch(At, q, y, mean, Ls, c, rho, idx, n):
    """(ELBO, d/dm, d/dL_s (lower), d/dc, d/drho) by the hand-derived formulas, vectorised (torch float64, any device):
    what the SGD loop below and the probe's torch column use"""
    a = At if idx is None else At[idx]
    qb = q if idx is None else q[idx]
    yb = y if idx is None else y[idx]
    b, m = a.shape
    low = torch.tril(Ls)
    sig2 = torch.nn.functional.softplus(rho, threshold=1e9) + MIN_NOISE
    w = a @ low
    r = yb - (c + a @ mean)
    e = r * r + qb + (w * w).sum(dim=1)
    ell = -HALF_LOG_2PI - 0.5 * torch.log(sig2) - e / (2.0 * sig2)
    d = low.diagonal()
    kl = 0.5 * ((low * low).sum() + (mean * mean).sum() - m - 2.0 * torch.log(d.abs()).sum())
    gmu = r / sig2
    g_m = (a.T @ gmu) / b - mean / n
    g_l = torch.tril((2.0 / b) * (a.T @ (w * (-0.5 / sig2)))) - (low - torch.diag(1.0 / d)) / n
    g_c = gmu.mean()
    g_rho = torch.sigmoid(rho) * (-0.5 / sig2 + e / (2.0 * sig2 * sig2)).mean()
    return ell.mean() - kl / n, g_m, g_l, g_c, g_rho


def sgd_loop(At, q, y, mean, Ls, c, rho, batches_per_epoch, lr, train_mean=True, train_noise=True, perturb=0.0):
    """Plain SGD on loss = -ELBO over the given index batches (a list per epoch), the full-data loss after every epoch
    (experiments/trainers.py:120-127).  ``perturb``: every gradient component is multiplied by 1 +- perturb, the signs
    alternating -- the rerun that measures how fast two correct loops diverge.  Returns (losses, mean, Ls, c, rho)."""
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
            _, g_m, g_l, g_c, g_rho = gradients_torch(At, q, y, mean, Ls, c, rho, idx, n)
            mean = mean - lr * (-jolt(g_m))
            Ls = Ls - lr * (-jolt(g_l))
            if train_mean:
                c = c - lr * (-jolt(g_c))
            if train_noise:
                rho = rho - lr * (-jolt(g_rho))
        losses.append(-float(gradients_torch(At, q, y, mean, Ls, c, rho, None, n)[0]))
    return losses, mean, Ls, float(c), float(rho)


def closed_form_optimum(At, y, c, rho):
    """(m*, L_s*) of the full-batch ELBO at fixed c and noise: S* = (I + A A^T / sigma^2)^-1, m* = S* A (y - c) / sigma^2,
    L_s* = chol(S*), with A = At^T"""
    sig2 = softplus(float(rho)) + MIN_NOISE
    A = At.T
    h = torch.eye(A.shape[0], dtype=torch.float64) + A @ A.T / sig2
    s = torch.linalg.inv(h)
    s = 0.5 * (s + s.T)
    m_star = torch.linalg.solve(h, A @ (y - c) / sig2)
    return m_star, torch.linalg.cholesky(s)


# ---- seeded inputs: integer draws and exactly rounded elementwise operations only (the same doubles on every machine) ----
def make_inputs(seed, n, m, b=None):
    """At ~ 0.3 N(0, 1), q = 0.05 + U, y ~ N(0, 1), m ~ 0.5 N(0, 1), L_s = 0.2 N(0, 1) below a diagonal 0.5 + U with
    alternating sign, c = 0.3, rho = -0.7; idx: b distinct rows, 37 apart (mod n), None when b is None"""
    g = torch.Generator().manual_seed(seed)
    At = 0.3 * _normal(g, (n, m))
    q = 0.05 + _uniform(g, (n,))
    y = _normal(g, (n,))
    mean = 0.5 * _normal(g, (m,))
    Ls = torch.tril(0.2 * _normal(g, (m, m)), diagonal=-1)
    sign = torch.where(torch.arange(m) % 3 == 2, -1.0, 1.0).double()
    Ls = Ls + torch.diag((0.5 + _uniform(g, (m,))) * sign)
    idx = None
    if b is not None:
        assert math.gcd(37, n) == 1 and b <= n
        idx = (seed % n + 37 * torch.arange(b, dtype=torch.int64)) % n
    return dict(At=At, q=q, y=y, mean=mean, Ls=Ls, c=0.3, rho=-0.7, idx=idx, n=n)


CASES = {f"m{_m}-b{_b}": (_m, _b, 700000 + 100 * _m + _b) for _m in (1, 2, 17, 33) for _b in (1, 2, 63, 65)}


def case_inputs(name):
    m, b, seed = CASES[name]
    return make_inputs(seed, N_FIXTURE, m, b)


def hashed(inp):
    """the tensors of a case that the fixture's SHA-256 covers, in its order"""
    return [inp[k] for k in ("At", "q", "y", "mean", "Ls", "idx")]


def evaluate_inputs(inp, majorant=False):
    return evaluate(inp["At"].numpy(), inp["q"].numpy(), inp["y"].numpy(), inp["mean"].numpy(), inp["Ls"].numpy(), inp["c"],
                    inp["rho"], None if inp["idx"] is None else inp["idx"].numpy(), inp["n"], majorant)


def truth(name):
    """the 50-digit output vector of a fixture case as (hi, lo), after checking that the inputs are the recorded ones"""
    return fixture_truth(TRUTH, name, hashed(case_inputs(name)))


_cpu_cache = {}


def cpu_case(name):
    """(inputs, fsum output vector, scale vector) of a fixture case, computed once and shared"""
    if name not in _cpu_cache:
        inp = case_inputs(name)
        _cpu_cache[name] = (inp, evaluate_inputs(inp), evaluate_inputs(inp, majorant=True))
    return _cpu_cache[name]
