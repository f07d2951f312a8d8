"""A per-element truth for the count-model additions, in the shape of tests/cost_truth.py: the negative binomial under the
exponential link (the pair with kernel instantiations of its own) and Gaussian/exp (the exponential link's value and slope
through the run-time-switch instantiation), written in mpmath (50 digits) as include/plship.h states them, on a grid of
(y, f) organised in named regimes; and a plain fp64 torch restatement of the cost on the host, duck-typed like the oracle's
costs, whose recorded error against the truth (tests/golden/count_cost_reference_errors.json) sets the bound.

  negative binomial, t = f - log r:   cost = r softplus(t) + y softplus(-t),   cost' = r sigma(t) - y sigma(-t)
  (= r log1p(mu / r) + y log1p(r / mu) and r (mu - y) / (r + mu) with mu = e^f; tests/test_count_cost_host.py holds the two
  forms to each other in mpmath)

Inputs are fp64 numbers taken exactly (r too; log r is mathematical).  A truth beyond the fp64 range is +-inf (or 0).

Regimes (a column is one regime; every row has its own y: 0, 1, 3, 25, 1e6, 0.5, 1/3):
  bulk      |f| <= 3
  root      e^f = y (1 +- 2^-k), k = 8..50 (f = -k for y = 0): the negative-binomial derivative cancels there
  lo_tail / hi_tail   -+30 ... -+700
  far       +-745, +-1e10, +-1e150, +-1e300: the link overflows or underflows; the negative binomial stays finite
  zero      +-0 and subnormals (for y = 1 a root too: e^0 = y, the negative-binomial derivative is exactly 0 there)

Error units.  Ulps of the truth, except
  root, and zero for the negative-binomial derivative (the formula cancels):
    negative binomial, derivative:  2^-53 (|r sigma(t)| + |y sigma(-t)|)
    Gaussian/exp, value and derivatives:  2^-53 (|T| + |dT/dp| p), p = e^f against y (as cost_truth's Gaussian/square root)
  far, Gaussian/exp: the larger of an ulp of the truth and |dT/dp| 2^-1074 -- at f = -745 the link value is a subnormal
    fp64 number (one step of 2^-1074 is 1 % of it), and Gaussian/exp is a function of that number; the negative binomial
    never forms it and keeps the ulp"""
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
PAIRS = ["negative_binomial/exp", "gaussian/exp"]
KINDS = T.KINDS
# the dispersion r, the noise variance: set b is r = 50, close to the Poisson limit
PARAMS = {"a": {"negative_binomial": (0.7,), "gaussian": (0.3,)}, "b": {"negative_binomial": (50.0,), "gaussian": (2.5,)}}
U = T.U
HUGE = 1e6  # |x| beyond which e^x is stated (inf / 0), not computed
# The selector problems of tests/step_fixtures.py: carrier values F = c_n V_j with |c_n| <= 8 and a jiggle of up to 1 + 2^-4.
# The probe rows must neither overflow nor land between 2^-1000 and 0 after the scaling by eta 2^p >= 2^-23
# (SelectorProblem.expected):
#   negative binomial/exp: G lies in [-y, r]; for y = 0 it is r sigma(t) ~ e^F, fine down to F = -640 (e^-640 = 2^-923) and
#     exactly 0 from F = -1e9 on, so |f| <= 75 or |f| >= 1e9 (the grid's +-1e10: value and derivative in their linear ends)
#   Gaussian/exp: G = (e^F - y) e^F / sigma2 ~ e^2F must stay finite and above 2^-970: |F| <= 255, |f| <= 30
SELECTOR_RANGE = {"negative_binomial/exp": lambda a: (a <= 75) | ((a >= 1e9) & (a <= 1e30)), "gaussian/exp": lambda a: a <= 30}
OWN_CARRIER_STREAM = True  # the carrier values and labels come from a generator of their own (seed + 4242)
MODES_AGREE = True  # both derivative modes are the same bits, through the same instantiation


def unit_kind(pair, kind, regime):
    if kind == "link":
        return "ulp"
    if pair == "negative_binomial/exp":
        return "cancel" if kind.startswith("deriv") and regime in ("root", "zero") else "ulp"
    return "cancel" if regime == "root" else "subnormal_link" if regime == "far" else "ulp"


# ---- the grid -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(pair, pset):
    """(y (N,), f (N, J), regimes (J names)): every row has its own y, a column is one regime; N and J are off every
    multiple of 4"""
    assert pair in PAIRS
    y = [0.0, 1.0, 3.0, 25.0, 1e6, 0.5, 1.0 / 3.0]
    cols = [("bulk", (lambda yy, v=v: v)) for v in (0.3, -0.3, 0.9, -0.9, 1.3, -1.3, 2.6, -2.6, 2.95, -2.95)]
    cols += [("root", (lambda yy, k=k, s=s: math.log(yy) + math.log1p(s * 2.0 ** -k) if yy > 0 else -float(k)))
             for k in (8, 20, 30, 40, 50) for s in (1, -1)]
    cols += [("hi_tail", (lambda yy, v=v: v)) for v in (30.0, 100.0, 300.0, 700.0)]
    cols += [("lo_tail", (lambda yy, v=v: -v)) for v in (30.0, 100.0, 300.0, 700.0)]
    cols += [("far", (lambda yy, v=v, s=s: s * v)) for v in (745.0, 1e10, 1e150, 1e300) for s in (1, -1)]
    cols += [("zero", (lambda yy, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.2250738585072014e-308)]
    while len(y) % 4 == 0 or len(y) % 2 == 0:
        y = y + [y[1]]
    while len(cols) % 4 == 0 or len(cols) % 2 == 0:
        cols = cols + [cols[len(cols) // 3]]
    f = np.array([[gen(yy) for _, gen in cols] for yy in y], dtype=np.float64)
    return np.array(y, dtype=np.float64), f, [r for r, _ in cols]


# ---- the truth ----------------------------------------------------------------------------------------------------------------
def _exp(x):
    """e^x as an mpf; stated beyond +-HUGE (0 below; above, the callers return their own special)"""
    return mp.mpf(0) if x < -HUGE else mp.exp(x)


def softplus(x):
    """log(1 + e^x) without forming e^|x|"""
    return (x if x > 0 else mp.mpf(0)) + mp.log1p(_exp(-abs(x)))


def sigma(x):
    e = _exp(-abs(x))
    return 1 / (1 + e) if x >= 0 else e / (1 + e)


def nb_softplus_form(r, y, f):
    """(value, derivative, r sigma(t), y sigma(-t)) in t = f - log r"""
    r, y, t = mp.mpf(r), mp.mpf(y), mp.mpf(f) - mp.log(mp.mpf(r))
    a, b = r * sigma(t), y * sigma(-t)
    return r * softplus(t) + (y * softplus(-t) if y != 0 else 0), a - b, a, b


def nb_mu_form(r, y, f):
    """the header's statement in mu = e^f: r log1p(mu / r) + y log1p(r / mu) and r (mu - y) / (mu (r + mu)) mu"""
    r, y, mu = mp.mpf(r), mp.mpf(y), mp.exp(mp.mpf(f))
    return r * mp.log1p(mu / r) + (y * mp.log1p(r / mu) if y != 0 else 0), r * (mu - y) / (mu * (r + mu)) * mu


def _gauss_from_p(kind, s2, y, p):
    e = p - y
    return e * e / (2 * s2) if kind == "value" else e / s2 * p  # (slope = p)


def point_truth(pair, pset, kind, y, f):
    """(T, cancel unit) of one fp64 point; T is an mpf, or a float special (+inf where e^f is beyond every range)"""
    cost = pair.split("/")[0]
    (p0,) = PARAMS[pset][cost]
    if kind == "link":
        if f > HUGE:
            return math.inf, None
        t = _exp(mp.mpf(f))
        return t, U * abs(t)
    if cost == "negative_binomial":
        v, d, a, b = nb_softplus_form(p0, y, f)
        return (v, U * abs(v)) if kind == "value" else (d, U * (abs(a) + abs(b)))
    if f > HUGE:  # Gaussian/exp: (inf - y)^2, (inf - y) inf
        return math.inf, None
    p, ym, s2 = _exp(mp.mpf(f)), mp.mpf(y), mp.mpf(p0)
    t = _gauss_from_p(kind, s2, ym, p)
    d = (p if p != 0 else mp.mpf(1)) * mp.mpf(2) ** -100
    sens = abs(_gauss_from_p(kind, s2, ym, p + d) - t) / d
    return t, (U * (abs(t) + sens * p), sens * mp.mpf(2) ** -1074)


@functools.lru_cache(maxsize=None)
def truth(pair, pset, kind):
    """dict of (N, J) fp64 arrays: hi + lo = the truth (hi alone for specials), unit = the regime's error unit"""
    y, f, regimes = grid(pair, pset)
    n, j = f.shape
    hi, lo, unit = np.zeros((n, j)), np.zeros((n, j)), np.zeros((n, j))
    for a in range(n):
        for b in range(j):
            t, cu = point_truth(pair, pset, kind, float(y[a]), float(f[a, b]))
            if isinstance(t, float):
                hi[a, b], lo[a, b], unit[a, b] = t, 0.0, math.nan
                continue
            hi[a, b], lo[a, b] = T._split(t)
            uk = unit_kind(pair, kind, regimes[b])
            cu, sub = cu if isinstance(cu, tuple) else (cu, 0)
            unit[a, b] = max(float(cu), 2.0 ** -1074) if uk == "cancel" else T._ulp(hi[a, b])
            if uk == "subnormal_link":
                unit[a, b] = max(unit[a, b], float(sub))
    return {"hi": hi, "lo": lo, "unit": unit}


errors = T.errors
by_regime = T.by_regime
bound = T.bound  # the project's rule, unchanged: the larger of 4x the recorded reference error and 4 units


def cells():
    return [(pair, pset) for pair in PAIRS for pset in PARAMS]


def applies(pair, kind):
    return True


# ---- the host restatement and the library's objects ----------------------------------------------------------------------------
class ExpLink:
    def __call__(self, y):
        return torch.exp(y)


class NegativeBinomialHostCost(O._Cost):
    """The cost restated plainly in fp64 torch (project code, not the reference's), in the form of the oracle's costs, so
    oracle.pls_oracle.PLS and train_pls take it unchanged."""

    observation_noise = None

    def __init__(self, y_train, link_function, dispersion):
        assert isinstance(link_function, ExpLink)
        self.y_train, self.link_function, self.dispersion = y_train, link_function, float(dispersion)

    def _t(self, f):
        return f - math.log(self.dispersion)

    def calculate_cost(self, f):
        t, y = self._t(f), self.y_train[:, None].to(f.dtype)
        zero = torch.zeros_like(t)
        return (self.dispersion * torch.logaddexp(zero, t) + y * torch.logaddexp(zero, -t)).sum(dim=0)

    def calculate_cost_derivative(self, f, force_autograd=False):
        t, y = self._t(f), self.y_train[:, None].to(f.dtype)
        return self.dispersion * torch.sigmoid(t) - y * torch.sigmoid(-t)


def host_cost(pair, pset, y):
    cost = pair.split("/")[0]
    (p0,) = PARAMS[pset][cost]
    if cost == "negative_binomial":
        return NegativeBinomialHostCost(y, ExpLink(), p0)
    return O.GaussianCost(p0, y, ExpLink())


def gpu_cost(P, pair, pset, y):
    cost = pair.split("/")[0]
    (p0,) = PARAMS[pset][cost]
    link = P.links.ExponentialLinkFunction()
    if cost == "negative_binomial":
        return P.costs.NegativeBinomialCost(y, link, p0)
    return P.costs.GaussianCost(p0, y, link)


def host_eval(pair, pset, kind):
    """the host restatement on the grid, per element: (N, J)"""
    y, f, _ = grid(pair, pset)
    yt, ft = torch.as_tensor(y), torch.as_tensor(f)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        if kind == "link":
            return host_cost(pair, pset, yt).link_function(ft).numpy()
        if kind == "value":  # the cost sums over rows: one row at a time
            rows = [host_cost(pair, pset, yt[a:a + 1]).calculate_cost(ft[a:a + 1]).reshape(-1) for a in range(len(y))]
            return torch.stack(rows).numpy()
        return host_cost(pair, pset, yt).calculate_cost_derivative(ft, force_autograd=kind == "deriv_autograd").numpy()
    finally:
        torch.set_default_dtype(prev)


def measure_reference():
    """{pair: {parameter set: {kind: {regime: the host restatement's largest error in the regime's unit}}}}"""
    out = {}
    for pair, pset in cells():
        regimes = grid(pair, pset)[2]
        for kind in KINDS:
            err = errors(host_eval(pair, pset, kind), truth(pair, pset, kind))
            out.setdefault(pair, {}).setdefault(pset, {})[kind] = by_regime(err, regimes)
    return out


def reference_errors():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count_cost_reference_errors.json")) as fh:
        return json.load(fh)


# ---- what the family batteries take (tests/test_gpu_family_cost_{train,elements,routes}.py) ---------------------------------------
CHECKPOINT = ("dispersion", 99.0)  # the attribute a checkpoint carries, and the value the model it is loaded into was built with
VALUE_TRUTH_FINITE = False  # (the column-sum test asserts nothing about the truth's values first)
check_elements = None  # nothing beyond both derivative modes being the same bits
ROUTE_PAIR = "negative_binomial/exp"  # its own compile-time instantiation: every route, both derivative modes
ROUTE_RUNTIME_PAIR = "gaussian/exp"  # the run-time-switch instantiation: the plain route and the small-rank routes
ROUTE_SMALL_RANK_SETS = "a"  # the parameter sets the small-rank shapes cycle through
TRAIN_DISPERSION = 3.0


def train_y(pr, n):
    """over-dispersed counts around exp(1 + f*): a gamma-mixed Poisson with shape r"""
    rate = torch.exp(1.0 + pr["fstar"])
    mix = torch.distributions.Gamma(torch.tensor(TRAIN_DISPERSION, dtype=torch.float64), torch.tensor(TRAIN_DISPERSION, dtype=torch.float64))
    torch.manual_seed(11 + n)
    return torch.poisson(rate * mix.sample((n,)))


def train_costs(P, y, dispersion=TRAIN_DISPERSION):
    return (NegativeBinomialHostCost(y, ExpLink(), dispersion),
            P.costs.NegativeBinomialCost(y, P.links.ExponentialLinkFunction(), dispersion))


def check_trained_cost(gc):
    assert gc.dispersion == TRAIN_DISPERSION
