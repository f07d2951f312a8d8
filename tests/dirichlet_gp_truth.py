"""The yardstick of the Dirichlet exact-GP tests: the label transform of Milios et al. 2018 in plain float64, the
per-class marginal log-likelihood with its gradient through LAPACK with the diagonal v_c + sigma_c (built on the closed
forms of tests/exact_gp_truth.py), the host restatement of the class probabilities (oracle/philox_ref + numpy +
math.fsum), and the case table of tests/golden/dirichlet_gp_truth.npz (50-digit values, written by
tests/golden/make_dirichlet_gp_truth.py)."""
import math
import os

import numpy as np
import torch

import exact_gp_truth as E
from oracle import philox_ref
from truth_common import _normal, _uniform, checksum, fixture_truth  # noqa: F401

EPS = E.EPS
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dirichlet_gp_truth.npz")
ALPHA_EPSILON = 0.01
# the issue's literals: a -> (v, y~)
LITERALS = {0.01: (4.61512051684126, -6.912730444408721), 1.01: (0.6881843912178163, -0.33414186475574004)}


def transform(labels, classes, alpha_epsilon=ALPHA_EPSILON):
    """(y~, v), both (C, n) float64, by math.log per entry"""
    labels = [int(v) for v in labels]
    y = torch.empty(classes, len(labels), dtype=torch.float64)
    v = torch.empty_like(y)
    for c in range(classes):
        for i, lab in enumerate(labels):
            a = alpha_epsilon + (1.0 if lab == c else 0.0)
            v[c, i] = math.log(1.0 / a + 1.0)
            y[c, i] = math.log(a) - 0.5 * v[c, i].item()
    return y, v


def mll_and_grad(kind, x, targets, fixed, ls, s, sigma, mean):
    """all classes: (out, scale), both (C, 4 + d); ls (C, d), s / sigma / mean (C); fixed (C, n) or None"""
    rows = [E.mll_and_grad(kind, x, targets[c], ls[c], float(s[c]), float(sigma[c]), float(mean[c]),
                           None if fixed is None else fixed[c]) for c in range(targets.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def host_evaluate(model):
    """``evaluate`` for train_exact_gp(likelihood="dirichlet"): the model's loss and raw gradient from this module"""
    out, _ = mll_and_grad(model.kind, model.x, model.transformed_targets, model.fixed_noise, model.lengthscale,
                          model.outputscale, model.noise, model.mean_constant)
    return model.chain_rule(torch.from_numpy(out))


# ---- the class probabilities --------------------------------------------------------------------------------------------
def softmax_rows(a):
    e = np.exp(a - a.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def proba_point(mu, var, samples, seed, step, shift=None):
    """(C): (1/S) sum_s softmax(mu + sqrt(max(var, 0)) z[s, :]), z the library's normal matrix of `step`; the sum over s by
    math.fsum.  shift(z) -> z' moves the normals (the tests derive their bar from such a move)."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    z = philox_ref.normal_matrix(samples, mu.shape[0], seed, step)
    if shift is not None:
        z = shift(z)
    p = softmax_rows(mu[None, :] + np.sqrt(np.maximum(var, 0.0))[None, :] * z)
    return np.array([math.fsum(p[:, c].tolist()) for c in range(mu.shape[0])]) / samples


def proba(mu, var, samples, seed, first_point=0, shift=None):
    """(t, C) from mu, var (C, t)"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    return np.stack([proba_point(mu[:, i], var[:, i], samples, seed, first_point + i, shift) for i in range(mu.shape[1])])


def longest_path_additions(samples):
    """additions on the longest path of the device's documented order: a lane adds 2 samples per pair for its
    ceil(pairs / 64) pairs (pairs = 4 ceil(S / 8)), then 6 butterfly levels"""
    pairs = 4 * ((samples + 7) // 8)
    return 2 * ((pairs + 63) // 64) + 6


def proba_bar(mu, var, samples, seed, first_point=0):
    """The bar of the device's probabilities, from the restatement alone: 16 x the change when every normal is moved by
    8 eps max(1, |z|) (away from 0), plus eps x the additions on the longest path (entries are <= 1)."""
    base = proba(mu, var, samples, seed, first_point)
    moved = proba(mu, var, samples, seed, first_point, lambda z: z + np.copysign(8.0 * EPS * np.maximum(1.0, np.abs(z)), z))
    return 16.0 * np.abs(moved - base).max() + EPS * longest_path_additions(samples)


# the five (mu, var) pairs of the quadrature condition (C = 2), at S = 4096 and seed 7
QUAD_PAIRS = (((0.0, 0.0), (1.0, 1.0)), ((1.5, -0.5), (0.25, 0.5)), ((-2.0, 1.0), (9.0, 16.0)), ((3.0, 0.0), (2.0, 0.1)),
              ((-0.3, 0.4), (4.0, 1.0)))
QUAD_SAMPLES, QUAD_SEED = 4096, 7


def quadrature(mu, var):
    """(E sigma(g), the standard error of the mean of S draws) for g ~ N(mu0 - mu1, var0 + var1), by mpmath.quad: the
    probability of class 0 of two classes, softmax_0 = sigma(f0 - f1)"""
    import mpmath as mp

    m, s = mp.mpf(mu[0]) - mp.mpf(mu[1]), mp.sqrt(mp.mpf(var[0]) + mp.mpf(var[1]))
    sig = lambda g: 1 / (1 + mp.exp(-g))  # noqa: E731
    pdf = lambda u: mp.exp(-u * u / 2) / mp.sqrt(2 * mp.pi)  # noqa: E731
    cuts = [-mp.inf, -8, -2, 0, 2, 8, mp.inf]
    e1 = mp.quad(lambda u: sig(m + s * u) * pdf(u), cuts)
    e2 = mp.quad(lambda u: sig(m + s * u) ** 2 * pdf(u), cuts)
    return float(e1), float(mp.sqrt((e2 - e1 * e1) / QUAD_SAMPLES))


# ---- the fixture's cases: name -> (kind, n, d, classes, seed) -----------------------------------------------------------
CASES = {}
for _n in (2, 65, 130):
    for _d in (1, 3):
        for _c in (2, 3):
            for _kind in (E.RBF, E.MATERN32):
                CASES[f"{E.KIND_NAMES[_kind]}-n{_n}-d{_d}-c{_c}"] = (_kind, _n, _d, _c, 700000 + 1000 * _n + 100 * _c + 10 * _d + _kind)


def case_inputs(name):
    """kind, x ~ N(0, I) (n, d), labels from an integer stream of the case's generator, (y~, v) in float64 rounded to
    float32 (the default of the package), and per class: lengthscale (0.5 + U) sqrt(d), outputscale 0.8 + U,
    sigma 0.05 + 0.2 U, mean U - 0.5 -- all distinct"""
    kind, n, d, classes, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = _normal(g, (n, d))
    labels = torch.randint(0, classes, (n,), generator=g, dtype=torch.int64)
    y, v = transform(labels.tolist(), classes)
    y, v = y.float().double(), v.float().double()
    ls = (0.5 + _uniform(g, (classes, d))) * d**0.5
    s = 0.8 + _uniform(g, (classes,))
    sigma = 0.05 + 0.2 * _uniform(g, (classes,))
    mean = _uniform(g, (classes,)) - 0.5
    return kind, x, labels, y, v, ls, s, sigma, mean


def truth(name):
    """the 50-digit outputs (C, 4 + d) of a case as (hi, lo) float64 pairs, after checking the regenerated inputs"""
    return fixture_truth(TRUTH, name, case_inputs(name)[1:])


_cpu_cache = {}


def cpu_case(name):
    """(out, scale, e_cpu), all (C, 4 + d): the LAPACK evaluation, its scales and its error against the 50 digits relative
    to the scale -- computed once and shared"""
    if name not in _cpu_cache:
        kind, x, _, y, v, ls, s, sigma, mean = case_inputs(name)
        out, mag = mll_and_grad(kind, x, y, v, ls, s, sigma, mean)
        hi, lo = truth(name)
        _cpu_cache[name] = (out, mag, E.relative_error(out, hi, lo, mag))
    return _cpu_cache[name]
