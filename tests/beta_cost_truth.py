"""A per-element truth for the Beta cost, in the shape of tests/count_cost_truth.py: the pairs beta/sigmoid (the pair with
kernel instantiations of its own) and beta/probit (the chain rule in the clipped link value, through the run-time-switch
instantiation), and the three device special functions (lgamma, digamma, X(x) = x digamma(x)), written in mpmath (50 digits)
as include/plship.h states them, on a grid of (z, f) organised in named regimes; and a plain fp64 torch restatement on the
host, duck-typed like the oracle's costs, whose recorded error against the truth
(tests/golden/beta_cost_reference_errors.json) sets the bound.

  mu = link(f), a = phi mu, b = phi (1 - mu):   cost = lgamma(a) + lgamma(b) - a z,   cost' = phi [psi(a) - psi(b) - z] mu'
  z = logit(y) is the library's second argument; the truth takes the fp64 z exactly (correctly rounded from the row's y).

Rows (y): 0.5, 0.01, 0.999, 1/3, 1e-9, 1 - 2^-30, 0.2.  Regimes of beta/sigmoid (a column is one regime):
  bulk      |f| <= 3
  centre    +-2^-k, k = 8..50: psi(a_b) - psi(a_s) cancels
  root      f* (1 +- 2^-k), f* the zero of the derivative for the row's z (+-2^-k where f* = 0)
  lo_tail / hi_tail   -+30, 100, 300, 700
  far       +-745, +-1e10, +-1e150, +-1e300: exp(-|f|) underflows; value and derivative stay finite
  zero      +-0 and subnormals
beta/probit: bulk, and wide: 3 < |f| <= 8 on both sides of the clip (|f| = 6.36 for the jitter 1e-10).

Error units, every regime (conditioning-aware: mu carries a rounding before the special functions see it).  With the smaller
and the bigger shape a_s <= a_b, mu_s <= mu_b, w = phi mu_s mu_b, X(x) = x psi(x):
  value   2^-53 [ |lgamma a_s| + |lgamma a_b| + |a z| + |X(a_s)| + |X(a_b)| ]
  deriv   2^-53 [ |mu_b X(a_s)| + |w psi(a_b)| + |w z| + mu_b a_s^2 psi'(a_s) + w a_b psi'(a_b) ]
beta/probit: the same two sums in (a, b) with the link's slope in place of mu_s mu_b, and, as cost_truth does it for
Bernoulli/probit, what a rounding of the link value does: 2^-53 (|dT/dp| S + |dT/dq| (1 + p)), S the size of the terms p is
formed from and q = 1 - p taken as a variable of its own (b = phi q inherits the ABSOLUTE rounding of p, so its relative error
is 2^-53 / q: next to the upper clip that is the whole error).
Special functions: an ulp of the truth; lgamma within 2^-8 of 1 or 2: 2^-53 |x - 1| |psi(x)| (or |x - 2|) where that is
larger; psi and X within 2^-8 of their zero 1.4616...: 2^-53 x psi'(x) and 2^-53 x |X'(x)| where larger."""
import functools
import json
import math
import os

import mpmath as mp
import numpy as np
import torch

import cost_truth as T
from oracle import pls_oracle as O

mp.mp.dps = 50
PAIRS = ["beta/sigmoid", "beta/probit"]
KINDS = ["value", "deriv_reference", "deriv_autograd"]
PARAMS = {"a": 0.3, "b": 400.0, "c": 3.0}  # both shapes below 1; Stirling range; lgamma's zeros at 1 and 2, psi's at 1.4616
JITTER = 1e-10
U = T.U
HUGE = 1e6  # |f| beyond which exp(-|f|) is stated (0), not computed
# The selector problems of tests/step_fixtures.py (their ``y`` holds the logits z, the library's second argument): carrier
# values F = c_n V_j with |c_n| <= 8 and a jiggle of up to 1 + 2^-4.  The probe rows must neither overflow nor land between
# 2^-1000 and 0 after the scaling by eta 2^p >= 2^-23 (SelectorProblem.expected):
#   beta/sigmoid: |G| <= 1 + phi |z| / 4, and G -> +-1 in the tails: any finite F will do; |f| <= 1e30 keeps F itself finite
#   beta/probit: G = phi (psi(a) - psi(b) - z) slope with slope ~ e^(-F^2 / 2) inside the clip and exactly 0 outside it
#     (|F| > 6.36): every F is fine
SELECTOR_RANGE = {"beta/sigmoid": lambda a: a <= 1e30, "beta/probit": lambda a: a <= 1e30}
OWN_CARRIER_STREAM = True  # the carrier values and logits come from a generator of their own (seed + 4242)
MODES_AGREE = True  # both derivative modes are the same bits, through the same instantiation
Y_ROWS = [0.5, 0.01, 0.999, 1.0 / 3.0, 1e-9, 1.0 - 2.0 ** -30, 0.2]
PSI_ROOT = mp.findroot(mp.digamma, 1.46)
SPECIALS = {"lgamma": 4, "digamma": 5, "xdigamma": 6}  # name: op of pls_debug_math


def logit(y):
    """z = log y - log1p(-y) of an fp64 y, correctly rounded"""
    y = mp.mpf(y)
    return float(mp.log(y) - mp.log1p(-y))


Z_ROWS = [logit(y) for y in Y_ROWS]


# ---- the grid -----------------------------------------------------------------------------------------------------------------
def _slope_sign(phi, z, f):
    """psi(a) - psi(b) - z: the derivative without its positive factor"""
    e = mp.exp(-abs(f))
    mu_s, mu_b = e / (1 + e), 1 / (1 + e)
    a, b = (mu_b, mu_s) if f >= 0 else (mu_s, mu_b)
    return mp.digamma(phi * a) - mp.digamma(phi * b) - z


@functools.lru_cache(maxsize=None)
def root(pset, z):
    """f*: the zero of the beta/sigmoid derivative for this z (psi(a) - psi(b) rises from -inf to +inf with f)"""
    phi, zm = mp.mpf(PARAMS[pset]), mp.mpf(z)
    if z == 0.0:
        return 0.0
    g = lambda f: _slope_sign(phi, zm, f)  # noqa: E731
    lo, hi = mp.mpf(-700), mp.mpf(700)
    for _ in range(40):  # bracket by bisection, then polish
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if g(mid) < 0 else (lo, mid)
    return float(mp.findroot(g, (lo, hi), solver="secant", tol=mp.mpf(10) ** -60))


@functools.lru_cache(maxsize=None)
def grid(pair, pset):
    """(z (N,), f (N, J), regimes (J names)): every row has its own z, a column is one regime; N and J are off every
    multiple of 4"""
    assert pair in PAIRS
    z = list(Z_ROWS)
    cols = [("bulk", (lambda zz, v=v: v)) for v in (0.3, -0.3, 0.9, -0.9, 1.3, -1.3, 2.6, -2.6, 2.95, -2.95)]
    if pair == "beta/sigmoid":
        cols += [("centre", (lambda zz, k=k, s=s: s * 2.0 ** -k)) for k in (8, 15, 22, 29, 36, 43, 50) for s in (1, -1)]
        cols += [("root", (lambda zz, k=k, s=s: root(pset, zz) * (1 + s * 2.0 ** -k) if zz != 0.0 else s * 2.0 ** -k))
                 for k in (8, 20, 30, 40, 50) for s in (1, -1)]
        cols += [("hi_tail", (lambda zz, v=v: v)) for v in (30.0, 100.0, 300.0, 700.0)]
        cols += [("lo_tail", (lambda zz, v=v: -v)) for v in (30.0, 100.0, 300.0, 700.0)]
        cols += [("far", (lambda zz, v=v, s=s: s * v)) for v in (745.0, 1e10, 1e150, 1e300) for s in (1, -1)]
        cols += [("zero", (lambda zz, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.2250738585072014e-308)]
    else:
        cols += [("wide", (lambda zz, v=v, s=s: s * v)) for v in (3.5, 4.5, 5.5, 6.0, 6.3, 6.4, 7.0, 8.0) for s in (1, -1)]
    while len(z) % 4 == 0 or len(z) % 2 == 0:
        z = z + [z[1]]
    while len(cols) % 4 == 0 or len(cols) % 2 == 0:
        cols = cols + [cols[len(cols) // 3]]
    f = np.array([[gen(zz) for _, gen in cols] for zz in z], dtype=np.float64)
    return np.array(z, dtype=np.float64), f, [r for r, _ in cols]


# ---- the truth ----------------------------------------------------------------------------------------------------------------
def X(x):
    return x * mp.digamma(x) if x != 0 else mp.mpf(-1)


def beta_ab_form(phi, z, a, b, slope):
    """the header's statement in (a, b) = (phi mu, phi (1 - mu)): (value, derivative)"""
    return mp.loggamma(a) + mp.loggamma(b) - a * z, phi * (mp.digamma(a) - mp.digamma(b) - z) * slope


def beta_logit_form(phi, z, f):
    """the dedicated pair as the header states it: (value, derivative, value unit, derivative unit)"""
    phi, z, f = mp.mpf(phi), mp.mpf(z), mp.mpf(f)
    sg = 1 if f >= 0 else -1
    if abs(f) > HUGE:  # e = 0: a_s = 0, lgamma(a_s) = -log a_s = |f| - log phi, X(a_s) = -1
        lg_s, lg_b = abs(f) - mp.log(phi), mp.loggamma(phi)
        az = phi * z if sg > 0 else mp.mpf(0)
        return lg_s + lg_b - az, mp.mpf(sg), U * (abs(lg_s) + abs(lg_b) + abs(az) + 1 + abs(X(phi))), U
    e = mp.exp(-abs(f))
    mu_s, mu_b = e / (1 + e), 1 / (1 + e)
    a_s, a_b, w = phi * mu_s, phi * mu_b, phi * mu_s * mu_b
    lg_s = mp.loggamma(1 + a_s) - (mp.log(phi) - abs(f) - mp.log1p(e))
    lg_b = mp.loggamma(a_b)
    az = (a_b if sg > 0 else a_s) * z
    xs, pb = X(a_s), mp.digamma(a_b)
    v = lg_s + lg_b - az
    d = sg * (w * pb - mu_b * xs) - w * z
    uv = U * (abs(lg_s) + abs(lg_b) + abs(az) + abs(xs) + abs(X(a_b)))
    ud = U * (abs(mu_b * xs) + abs(w * pb) + abs(w * z) + mu_b * a_s * a_s * mp.polygamma(1, a_s) + w * a_b * mp.polygamma(1, a_b))
    return v, d, uv, ud


def _probit_from_p(phi, z, kind, p, q, slope):
    a, b = phi * p, phi * q
    v, d = beta_ab_form(phi, z, a, b, slope)
    return v if kind == "value" else d


def point_truth(pair, pset, kind, z, f):
    """(T, unit) of one fp64 point (T an mpf)"""
    phi = mp.mpf(PARAMS[pset])
    if pair == "beta/sigmoid":
        v, d, uv, ud = beta_logit_form(phi, z, f)
        return (v, uv) if kind == "value" else (d, ud)
    zm = mp.mpf(z)
    raw, p, slope, clipped, s = T.link_truth("probit", f, JITTER)
    q = 1 - p
    t = _probit_from_p(phi, zm, kind, p, q, slope)
    a, b = phi * p, phi * q
    if kind == "value":
        terms = abs(mp.loggamma(a)) + abs(mp.loggamma(b)) + abs(a * zm) + abs(X(a)) + abs(X(b))
    else:
        terms = phi * slope * (abs(mp.digamma(a)) + abs(mp.digamma(b)) + abs(zm) + a * mp.polygamma(1, a) + b * mp.polygamma(1, b))
    sens = mp.mpf(0)
    if not clipped:
        d = p * mp.mpf(2) ** -100
        sens = abs(_probit_from_p(phi, zm, kind, p + d, q, slope) - t) / d
    d = q * mp.mpf(2) ** -100
    sens_q = abs(_probit_from_p(phi, zm, kind, p, q + d, slope) - t) / d
    return t, U * (terms + sens * s + sens_q * (1 + p))


@functools.lru_cache(maxsize=None)
def truth(pair, pset, kind):
    """dict of (N, J) fp64 arrays: hi + lo = the truth, unit = the error unit"""
    z, f, regimes = grid(pair, pset)
    n, j = f.shape
    hi, lo, unit = np.zeros((n, j)), np.zeros((n, j)), np.zeros((n, j))
    for a in range(n):
        for b in range(j):
            t, cu = point_truth(pair, pset, "value" if kind == "value" else "deriv", float(z[a]), float(f[a, b]))
            hi[a, b], lo[a, b] = T._split(t)
            unit[a, b] = max(float(cu), 2.0 ** -1074)
    return {"hi": hi, "lo": lo, "unit": unit}


errors = T.errors
by_regime = T.by_regime
bound = T.bound  # the project's rule, unchanged: the larger of 4x the recorded reference error and 4 units


def cells():
    return [(pair, pset) for pair in PAIRS for pset in PARAMS]


def applies(pair, kind):
    return True


# ---- the special functions ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_points(name):
    """(x (K,), regimes (K names)): log-spaced over 1e-300 .. 1e300 (digamma: from 1), the pieces' seams, and dense around 1,
    the zero of psi and 2"""
    g = np.random.default_rng(SPECIALS[name])
    lo = 0.0 if name == "digamma" else -300.0
    parts = [("wide", 10.0 ** g.uniform(lo, 300.0, 700)), ("decades", 10.0 ** g.uniform(max(lo, -3.0), 3.0, 700)),
             ("seams", np.concatenate([g.uniform(1.0 if name == "digamma" else 0.1, 12.0, 600),
                                       np.array([0.75, 1.25, 1.75, 3.0, 8.0, 10.0, 2.0, 1.0])]).clip(1.0 if name == "digamma" else 0.0))]
    for label, c in (("near_1", 1.0), ("near_root", float(PSI_ROOT)), ("near_2", 2.0)):
        k = g.integers(8, 50, 300)
        pts = c + g.uniform(-1.0, 1.0, 300) * 2.0 ** -k.astype(np.float64)
        parts.append((label, np.maximum(pts, 1.0) if name == "digamma" else pts))
    x = np.concatenate([p for _, p in parts])
    return x, [r for r, p in parts for _ in range(len(p))]


def special_point_truth(name, x):
    xm = mp.mpf(x)
    if name == "lgamma":
        t, unit = mp.loggamma(xm), mp.mpf(0)
        for zero in (1, 2):
            if abs(xm - zero) < mp.mpf(2) ** -8:
                unit = U * abs(xm - zero) * abs(mp.digamma(xm))
    else:
        psi, tri = mp.digamma(xm), mp.polygamma(1, xm)
        t = psi if name == "digamma" else xm * psi
        # the conditioning unit everywhere, not only next to the zero of psi (a window would leave the points of the wide
        # regimes that fall near it, but outside the window, with an ulp of a small psi, and one such point sets the regime's bound)
        unit = U * xm * (tri if name == "digamma" else abs(psi + xm * tri))
    return t, unit


@functools.lru_cache(maxsize=None)
def special_truth(name):
    x, _ = special_points(name)
    hi, lo, unit = np.zeros((len(x), 1)), np.zeros((len(x), 1)), np.zeros((len(x), 1))
    for i, v in enumerate(x):
        t, cu = special_point_truth(name, float(v))
        hi[i, 0], lo[i, 0] = T._split(t)
        unit[i, 0] = max(T._ulp(hi[i, 0]), float(cu))
    return {"hi": hi, "lo": lo, "unit": unit}


def special_by_regime(err, regimes):
    out = {}
    for e, r in zip(np.asarray(err).reshape(-1), regimes):
        out[r] = max(out.get(r, 0.0), float(e))
    return out


def special_host(name, x):
    xt = torch.as_tensor(x, dtype=torch.float64)
    return (torch.lgamma(xt) if name == "lgamma" else torch.digamma(xt) if name == "digamma" else xt * torch.digamma(xt)).numpy()


# ---- the host restatement and the library's objects ----------------------------------------------------------------------------
class SigmoidLink:
    def __call__(self, y):
        return torch.sigmoid(y)


class ProbitLink:
    def __call__(self, y):
        return (0.5 * (1 + torch.erf(y / math.sqrt(2.0)))).clip(JITTER, 1 - JITTER)


def _xpsi(x):
    """X(x) = x psi(x), = -1 + x psi(1 + x) below 1"""
    return torch.where(x < 1, -1 + x * torch.digamma(1 + x), x * torch.digamma(x.clamp(min=0.5)))


class BetaHostCost(O._Cost):
    """The cost restated plainly in fp64 torch (project code, not the reference's), in the form of the oracle's costs, so
    oracle.pls_oracle.PLS and train_pls take it unchanged.  ``z_train`` holds the logits of the observed proportions."""

    observation_noise = None

    def __init__(self, z_train, link_function, precision):
        assert isinstance(link_function, (SigmoidLink, ProbitLink))
        self.z_train, self.link_function, self.precision = z_train, link_function, float(precision)
        self.y_train = torch.sigmoid(z_train)

    def _shapes(self, f):
        e = torch.exp(-f.abs())
        mu_b = 1 / (1 + e)
        mu_s = e * mu_b
        return e, mu_s, mu_b, self.precision * mu_s, self.precision * mu_b

    def calculate_cost(self, f):
        z, phi = self.z_train[:, None].to(f.dtype), self.precision
        if isinstance(self.link_function, ProbitLink):
            p = self.link_function(f)
            a, b = phi * p, phi * (1 - p)
            return (torch.lgamma(a) + torch.lgamma(b) - a * z).sum(dim=0)
        e, mu_s, mu_b, a_s, a_b = self._shapes(f)
        log_as = (math.log(phi) - f.abs()) - torch.log1p(e)
        return ((torch.lgamma(1 + a_s) - log_as) + torch.lgamma(a_b) - torch.where(f >= 0, a_b, a_s) * z).sum(dim=0)

    def calculate_cost_derivative(self, f, force_autograd=False):
        z, phi = self.z_train[:, None].to(f.dtype), self.precision
        if isinstance(self.link_function, ProbitLink):
            raw = 0.5 * (1 + torch.erf(f / math.sqrt(2.0)))
            inside = (raw >= JITTER) & (raw <= 1 - JITTER)
            slope = torch.where(inside, torch.exp(-0.5 * f * f) / math.sqrt(2 * math.pi), torch.zeros_like(f))
            p = raw.clip(JITTER, 1 - JITTER)
            return phi * (torch.digamma(phi * p) - torch.digamma(phi * (1 - p)) - z) * slope
        e, mu_s, mu_b, a_s, a_b = self._shapes(f)
        d = mu_s * _xpsi(a_b) - mu_b * _xpsi(a_s)
        return torch.where(f >= 0, d, -d) - (a_s * mu_b) * z


def _phi(pset):
    return PARAMS[pset]


def host_cost(pair, pset, z):
    return BetaHostCost(z, SigmoidLink() if pair == "beta/sigmoid" else ProbitLink(), _phi(pset))


def gpu_cost(P, pair, pset, z):
    link = P.links.SigmoidLinkFunction() if pair == "beta/sigmoid" else P.links.ProbitLinkFunction()
    return P.costs.BetaCost.from_logits(z, link, _phi(pset))


def host_eval(pair, pset, kind):
    """the host restatement on the grid, per element: (N, J)"""
    z, f, _ = grid(pair, pset)
    zt, ft = torch.as_tensor(z), torch.as_tensor(f)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        if kind == "value":  # the cost sums over rows: one row at a time
            rows = [host_cost(pair, pset, zt[a:a + 1]).calculate_cost(ft[a:a + 1]).reshape(-1) for a in range(len(z))]
            return torch.stack(rows).numpy()
        return host_cost(pair, pset, zt).calculate_cost_derivative(ft, force_autograd=kind == "deriv_autograd").numpy()
    finally:
        torch.set_default_dtype(prev)


def measure_reference():
    """{pair: {parameter set: {kind: {regime: the host restatement's largest error in the regime's unit}}},
    "special": {function: {regime: ...}}}"""
    out = {}
    for pair, pset in cells():
        regimes = grid(pair, pset)[2]
        for kind in KINDS:
            err = errors(host_eval(pair, pset, kind), truth(pair, pset, kind))
            out.setdefault(pair, {}).setdefault(pset, {})[kind] = by_regime(err, regimes)
    for name in SPECIALS:
        x, regimes = special_points(name)
        err = errors(special_host(name, x).reshape(-1, 1), special_truth(name))
        out.setdefault("special", {})[name] = special_by_regime(err, regimes)
    return out


def reference_errors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beta_cost_reference_errors.json")) as fh:
        return json.load(fh)


# ---- what the family batteries take (tests/test_gpu_family_cost_{train,elements}.py) and the route tests ---------------------------
CHECKPOINT = ("precision", 99.0)  # the attribute a checkpoint carries, and the value the model it is loaded into was built with
VALUE_TRUTH_FINITE = True  # the column-sum test asserts it before it sums
check_elements = None  # nothing beyond both derivative modes being the same bits
ROUTE_PAIR = "beta/sigmoid"  # its own compile-time instantiation: every route, both derivative modes
ROUTE_RUNTIME_PAIR = "beta/probit"  # the run-time-switch instantiation: the plain route and the small-rank routes
ROUTE_SMALL_RANK_SETS = "a"  # the parameter sets the small-rank shapes cycle through
TRAIN_PRECISION = 8.0


def train_y(pr, n):
    """proportions scattered around sigmoid(1.5 f*) with precision phi"""
    mu = torch.sigmoid(1.5 * pr["fstar"])
    torch.manual_seed(11 + n)
    return torch.distributions.Beta(TRAIN_PRECISION * mu, TRAIN_PRECISION * (1 - mu)).sample().clamp(1e-6, 1 - 1e-6)


def train_costs(P, y, precision=TRAIN_PRECISION):
    gc = P.costs.BetaCost(y, P.links.SigmoidLinkFunction(), precision)
    return BetaHostCost(gc.y_device().cpu(), SigmoidLink(), precision), gc  # (the very logits the library gets)


def check_trained_cost(gc):
    assert gc.precision == TRAIN_PRECISION
