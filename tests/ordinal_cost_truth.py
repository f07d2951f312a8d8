"""A per-element truth for the ordinal cost (cumulative logit under the identity link, the pair with kernel instantiations of
its own), in the shape of tests/count_cost_truth.py: written in mpmath (50 digits) as include/plship.h states it, on a grid of
(label, f) organised in named regimes; and a plain fp64 torch restatement of the cost on the host, duck-typed like the oracle's
costs, whose recorded error against the truth (tests/golden/ordinal_cost_reference_errors.json) sets the bound.

  label k between lo = b_k and hi = b_(k+1) (b_0 = -inf, b_K = +inf):
  cost = softplus(f - hi) + softplus(lo - f),   cost' = sigma(f - hi) - sigma(lo - f)
  (the negative log-likelihood -log[sigma(hi - f) - sigma(lo - f)] without its f-independent term -log(1 - e^-(hi - lo));
  tests/test_ordinal_cost_host.py holds the two forms to each other in mpmath)

Inputs are fp64 numbers taken exactly (the cutpoints too).

Parameter sets: a = (-1.5, -0.25, 0.5, 2.0), five categories; b = (-0.001, 0.002, +inf, +inf), three categories with a narrow
middle one.  Rows: one per label.  Regimes (a column is one regime):
  bulk      |f| <= 3
  cut       f = lo or hi of the row's label, +- 2^-k, k = 8..50 (an edge label, which has one finite cutpoint of its own, takes
            its neighbour's other finite cutpoint as the second)
  root      interior labels: the interval's midpoint +- 2^-k times its width, where the derivative cancels; the two edge labels
            have no root: -k (bottom) and +k (top), their own side
  lo_tail / hi_tail   -+30 ... -+700
  far       +-745, +-1e10, +-1e150, +-1e300: the value is linear in |f|, or underflows gradually to 0 for an edge label on its
            own side; the derivative is +-1 or +-0
  zero      +-0 and subnormals

Error units.  Ulps of the truth (floor 2^-1074), except the derivative of an interior label in bulk, cut, root and zero, where
the two sigmoids cancel: 2^-53 (|sigma(f - hi)| + |sigma(lo - f)|).  No unit departs from the issue's plan."""
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
PAIRS = ["ordinal/identity"]
KINDS = ["value", "deriv_reference", "deriv_autograd"]
INF = math.inf
# the cutpoints: set b is three categories with the narrow middle one (two of the four cutpoint slots are +inf)
PARAMS = {"a": (-1.5, -0.25, 0.5, 2.0), "b": (-0.001, 0.002, INF, INF)}
U = T.U
HUGE = 1e6  # |x| beyond which e^x is stated (0), not computed
CANCEL_REGIMES = ("bulk", "cut", "root", "zero")
# The selector problems of tests/step_fixtures.py: carrier values F = c_n V_j with |c_n| <= 8 and a jiggle of up to 1 + 2^-4.
# The probe rows must neither overflow nor land between 2^-1000 and 0 after the scaling by eta 2^p >= 2^-23
# (SelectorProblem.expected):
#   ordinal/identity: G lies in (-1, 1); in an edge label's own tail it is +-sigma(-|F - b|) ~ e^-|F|, fine down to
#     |F| = 640 (e^-640 = 2^-923) and exactly 0 from |F| = 1e9 on (e^-|F| underflows from 745), so |f| <= 75 or |f| >= 1e9
#     (the grid's +-1e10: value and derivative in their linear ends), as for the negative binomial
SELECTOR_RANGE = {"ordinal/identity": lambda a: (a <= 75) | ((a >= 1e9) & (a <= 1e30))}
OWN_CARRIER_STREAM = True  # the carrier values and labels come from a generator of their own (seed + 4242)
MODES_AGREE = True  # both derivative modes are the same bits, through the same instantiation


def categories(pset):
    return 1 + sum(math.isfinite(b) for b in PARAMS[pset])


def cuts(pset, label):
    """(lo, hi) of a label: floats, -inf / +inf at the two ends"""
    b = (-INF,) + tuple(PARAMS[pset])[:categories(pset) - 1] + (INF,)
    k = int(label)
    assert k == label and 0 <= k < categories(pset), label
    return b[k], b[k + 1]


def interior(pset, label):
    lo, hi = cuts(pset, label)
    return math.isfinite(lo) and math.isfinite(hi)


def finite_cuts(pset, label):
    """the label's two cutpoints, an infinite one replaced by the neighbour's other finite cutpoint"""
    lo, hi = cuts(pset, label)
    if not math.isfinite(lo):
        lo, hi = hi, cuts(pset, label + 1)[1]
    if not math.isfinite(hi):
        lo, hi = cuts(pset, label - 1)[0], lo
    return lo, hi


def unit_kind(pset, kind, regime, label):
    return "cancel" if kind.startswith("deriv") and regime in CANCEL_REGIMES and interior(pset, label) else "ulp"


# ---- the grid -----------------------------------------------------------------------------------------------------------------
def _root_point(pset, label, k, s):
    lo, hi = cuts(pset, label)
    if not math.isfinite(lo):
        return -float(k)
    if not math.isfinite(hi):
        return float(k)
    return (lo + hi) / 2 + s * 2.0 ** -k * (hi - lo)


@functools.lru_cache(maxsize=None)
def grid(pair, pset):
    """(y (N,), f (N, J), regimes (J names)): one row per label, a column is one regime; N and J are off every multiple of
    4"""
    assert pair in PAIRS
    y = [float(k) for k in range(categories(pset))]
    cols = [("bulk", (lambda yy, v=v: v)) for v in (0.3, -0.3, 0.9, -0.9, 1.3, -1.3, 2.6, -2.6, 2.95, -2.95)]
    cols += [("cut", (lambda yy, k=k, s=s, w=w: finite_cuts(pset, yy)[w] + s * 2.0 ** -k))
             for w in (0, 1) for k in (8, 20, 30, 40, 50) for s in (1, -1)]
    cols += [("root", (lambda yy, k=k, s=s: _root_point(pset, yy, k, s))) for k in (8, 20, 30, 40, 50) for s in (1, -1)]
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
    """e^x as an mpf; stated (0) below -HUGE"""
    return mp.mpf(0) if x < -HUGE else mp.exp(x)


def softplus(x):
    """log(1 + e^x) without forming e^|x|; exactly 0 at -inf"""
    if x == -mp.inf:
        return mp.mpf(0)
    return (x if x > 0 else mp.mpf(0)) + mp.log1p(_exp(-abs(x)))


def sigma(x):
    if x == -mp.inf:
        return mp.mpf(0)
    e = _exp(-abs(x))
    return 1 / (1 + e) if x >= 0 else e / (1 + e)


def ordinal_form(lo, hi, f):
    """(value, derivative, sigma(f - hi), sigma(lo - f)) as the header states them"""
    lo, hi, f = mp.mpf(lo), mp.mpf(hi), mp.mpf(f)
    a, b = sigma(f - hi), sigma(lo - f)
    return softplus(f - hi) + softplus(lo - f), a - b, a, b


def full_nll(lo, hi, f):
    """-log P(y = k | f) = -log[sigma(hi - f) - sigma(lo - f)], from the definition"""
    lo, hi, f = mp.mpf(lo), mp.mpf(hi), mp.mpf(f)
    upper = mp.mpf(1) if hi == mp.inf else 1 / (1 + mp.exp(f - hi))
    lower = mp.mpf(0) if lo == -mp.inf else 1 / (1 + mp.exp(f - lo))
    return -mp.log(upper - lower)


def probabilities(cutpoints, f):
    """[P(y = k | f)] over the categories, mpf"""
    b = [mp.mpf(c) for c in cutpoints if math.isfinite(c)]
    cum = [mp.mpf(0)] + [1 / (1 + mp.exp(mp.mpf(f) - c)) for c in b] + [mp.mpf(1)]
    return [cum[k + 1] - cum[k] for k in range(len(b) + 1)]


def point_truth(pair, pset, kind, y, f):
    """(T, cancel unit) of one fp64 point; T is an mpf"""
    lo, hi = cuts(pset, y)
    v, d, a, b = ordinal_form(lo, hi, f)
    return (v, U * abs(v)) if kind == "value" else (d, U * (abs(a) + abs(b)))


@functools.lru_cache(maxsize=None)
def truth(pair, pset, kind):
    """dict of (N, J) fp64 arrays: hi + lo = the truth, unit = the regime's error unit"""
    y, f, regimes = grid(pair, pset)
    n, j = f.shape
    hi, lo, unit = np.zeros((n, j)), np.zeros((n, j)), np.zeros((n, j))
    for a in range(n):
        for b in range(j):
            t, cu = point_truth(pair, pset, kind, float(y[a]), float(f[a, b]))
            hi[a, b], lo[a, b] = T._split(t)
            cancel = unit_kind(pset, kind, regimes[b], float(y[a])) == "cancel"
            unit[a, b] = max(float(cu), 2.0 ** -1074) if cancel else T._ulp(hi[a, b])
    return {"hi": hi, "lo": lo, "unit": unit}


errors = T.errors
by_regime = T.by_regime
bound = T.bound  # the project's rule, unchanged: the larger of 4x the recorded reference error and 4 units


def cells():
    return [(pair, pset) for pair in PAIRS for pset in PARAMS]


def applies(pair, kind):
    return True


# ---- the host restatement and the library's objects ----------------------------------------------------------------------------
class OrdinalHostCost(O._Cost):
    """The cost restated plainly in fp64 torch (project code, not the reference's), in the form of the oracle's costs, so
    oracle.pls_oracle.PLS and train_pls take it unchanged.  ``cutpoints``: the finite ones, ascending."""

    observation_noise = None

    def __init__(self, y_train, link_function, cutpoints):
        assert isinstance(link_function, O.IdentityLink)
        self.y_train, self.link_function = y_train, link_function
        self.cutpoints = [float(c) for c in cutpoints if math.isfinite(float(c))]

    def _cuts(self, f):
        b = torch.tensor([-INF] + self.cutpoints + [INF], dtype=f.dtype)
        k = self.y_train.to(torch.long)
        return b[k][:, None], b[k + 1][:, None]

    def calculate_cost(self, f):
        lo, hi = self._cuts(f)
        zero = torch.zeros_like(f)
        return (torch.logaddexp(zero, f - hi) + torch.logaddexp(zero, lo - f)).sum(dim=0)

    def calculate_cost_derivative(self, f, force_autograd=False):
        lo, hi = self._cuts(f)
        return torch.sigmoid(f - hi) - torch.sigmoid(lo - f)


def host_cost(pair, pset, y):
    return OrdinalHostCost(y, O.IdentityLink(), PARAMS[pset])


def gpu_cost(P, pair, pset, y):
    """the library's object on raw labels (OrdinalCost itself refuses labels outside [0, K - 1]; the grid's are inside)"""
    k = categories(pset)
    return P.costs.OrdinalCost(y, P.links.IdentityLinkFunction(), cutpoints=list(PARAMS[pset])[:k - 1])


def host_eval(pair, pset, kind):
    """the host restatement on the grid, per element: (N, J)"""
    y, f, _ = grid(pair, pset)
    yt, ft = torch.as_tensor(y), torch.as_tensor(f)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
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
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ordinal_cost_reference_errors.json")) as fh:
        return json.load(fh)


# ---- what the family batteries take (tests/test_gpu_family_cost_{train,elements,routes}.py) ---------------------------------------
CHECKPOINT = ("cutpoints", [-3.0, 0.125, 7.0])  # the attribute a checkpoint carries, and the value the model it is loaded into was built with
VALUE_TRUTH_FINITE = True  # the column-sum test asserts it before it sums
ROUTE_PAIR = "ordinal/identity"  # its own compile-time instantiation: every route, both derivative modes
ROUTE_RUNTIME_PAIR = None  # no pair of this family goes through the run-time-switch instantiation
ROUTE_SMALL_RANK_SETS = "ab"  # the parameter sets the small-rank shapes cycle through: the labels differ from lane to lane here
TRAIN_THRESHOLDS = [-1.5, -0.25, 1.0]  # four grades cut from the noisy latent


def train_y(pr, n):
    g = torch.Generator().manual_seed(11 + n)
    uniform = torch.rand(n, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)
    latent = 1.5 * pr["fstar"].reshape(-1).double() + torch.log(uniform) - torch.log1p(-uniform)  # logistic noise
    return torch.bucketize(latent, torch.tensor(TRAIN_THRESHOLDS, dtype=torch.float64)).double()


def train_costs(P, y, cutpoints=None):
    if cutpoints is None:
        cutpoints = P.costs.OrdinalCost.cutpoints_from_labels(y, num_categories=len(TRAIN_THRESHOLDS) + 1)
    return OrdinalHostCost(y, O.IdentityLink(), cutpoints), P.costs.OrdinalCost(y, P.links.IdentityLinkFunction(), cutpoints=cutpoints)


def check_trained_cost(gc):
    assert len(set(gc.y_train.tolist())) == len(TRAIN_THRESHOLDS) + 1


def check_elements(got, pset):
    assert all((np.abs(got["deriv_reference", strided]) <= 1).all() for strided in (False, True)), "the derivative leaves [-1, 1]"
