"""A per-element truth for the Gamma cost (log link: the pair gamma/exp, with kernel instantiations of its own), in the shape of
tests/ordinal_cost_truth.py: written in mpmath (50 digits) as include/plship.h states it, on a grid of (z, f) organised in
named regimes; and a plain fp64 torch restatement of the device formulas on the host -- the two-sum correction of t = z - f
included -- duck-typed like the oracle's costs, whose recorded error against the truth
(tests/golden/gamma_cost_reference_errors.json) sets the bound.

  z = log y is the library's second argument, k the shape;  t = z - f:
  cost = k (e^t - t),   cost' = -k expm1(t)

Inputs are fp64 numbers taken exactly, and t is the exact real z - f: where the fp64 subtraction rounds, the truth does not.

Parameter sets: a: k = 2.5; b: a strongly skewed k = 0.05.  Rows (z): 0.3, -0.7, 2.5, 29.7, -29.9, 11.3, and 3 x 2^-1023, next
to which a difference is subnormal; all with |z| <= 30 (below).  Regimes (a column is one regime; f is formed in fp64 from
the row's z and the regime's t, so t is met up to the rounding of f):
  bulk      |t| <= 30
  root      f = z (1 +- eps), eps = 2^-52 (one ulp), 2^-50, 2^-40, 2^-30, 1e-6: z - f is exact and tiny, the derivative is
            -k t there; f = z (t = 0: the value is k, the derivative 0); f = z +- 5e-324 (t subnormal on the last row)
  round     |t| = 120.7, 333.3, 650.4, 700.4, both signs: z and f differ in size and the subtraction rounds -- uncorrected,
            that alone is up to a few hundred ulps of e^t
  over      t = 709.7, 709.78 (finite) and 709.79, 710, 1e6 (e^t rounds to +inf: value +inf, derivative -inf)
  under     t = -36, -38 (expm1 reaches -1), -745, -746 (e^t leaves the subnormals), -1e9, -1e300: value -k t, derivative k
  nonfinite f = -inf (+inf, -inf), f = +inf (+inf, k), f = NaN (NaN, NaN)
A non-finite z cannot be a row: the selector problems of tests/step_fixtures.py draw their labels from the rows and need a
finite G.  tests/test_gamma_cost_host.py (restatement) and tests/test_gpu_gamma_cost_elements.py (library) hold z = +-inf and
NaN to point_truth on rows of their own.

Error units: an ulp of the truth (floor 2^-1074) in every regime, value and derivative: there is no cancel unit, which is what
expm1 and the corrected t are for."""
import functools
import json
import math
import os

import mpmath as mp
import numpy as np
import torch

import cost_truth as T
from count_cost_truth import ExpLink
from oracle import pls_oracle as O

mp.mp.dps = 50
PAIRS = ["gamma/exp"]
KINDS = ["value", "deriv_reference", "deriv_autograd"]
INF = math.inf
PARAMS = {"a": 2.5, "b": 0.05}
U = T.U
HUGE = 1e6  # |t| beyond which e^t is stated (0 or +inf), not computed
EXP_OVERFLOW = mp.mpf(2) ** 1024 * (1 - mp.mpf(2) ** -54)  # from here e^t rounds to +inf: "above the exponential's range"
Z_ROWS = [0.3, -0.7, 2.5, 29.7, -29.9, 11.3, 3 * 2.0 ** -1023]
# The selector problems of tests/step_fixtures.py (their ``y`` holds z = log y, the library's second argument, drawn from the
# rows above: |z| <= 30): carrier values F = c_n V_j with |c_n| <= 8 and a jiggle of up to 1 + 2^-4.  The probe rows must neither
# overflow nor land between 2^-1000 and 0 after the scaling by eta 2^p >= 2^-23 (SelectorProblem.expected):
#   G = -k expm1(z - F).  |f| <= 60 gives |F| <= 510 and |t| <= 540: k e^t <= 2.5 x 2^780, times 2^p <= 4 far inside 2^1000;
#   towards -t G tends to k; at the root |G| ~ k |t| >= 0.05 x 2^-53 |z| (|F| >= 1e-30: t is 0 or at least an ulp of z or F)
SELECTOR_RANGE = {"gamma/exp": lambda a: a <= 60}
OWN_CARRIER_STREAM = True  # the carrier values and logarithms come from a generator of their own (seed + 4242)
MODES_AGREE = True  # both derivative modes are the same bits, through the same instantiation


# ---- the grid -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid(pair, pset):
    """(z (N,), f (N, J), regimes (J names)): every row has its own z, a column is one regime; N and J are off every
    multiple of 4"""
    assert pair in PAIRS
    z = list(Z_ROWS)
    at = lambda t: (lambda zz, t=t: zz - t)  # noqa: E731  (f for a target t; rounds where z and t differ in size)
    cols = [("bulk", at(s * v)) for v in (0.3, 0.9, 1.0, 2.6, 7.5, 17.3, 22.1, 30.0) for s in (1, -1)]
    cols += [("root", (lambda zz, e=e, s=s: zz * (1 + s * e))) for e in (2.0 ** -52, 2.0 ** -50, 2.0 ** -40, 2.0 ** -30, 1e-6) for s in (1, -1)]
    cols += [("root", (lambda zz: zz)), ("root", (lambda zz: zz + 5e-324)), ("root", (lambda zz: zz - 5e-324))]
    cols += [("round", at(s * v)) for v in (120.7, 333.3, 650.4, 700.4) for s in (1, -1)]
    cols += [("over", at(v)) for v in (709.7, 709.78, 709.79, 710.0, 1e6)]
    cols += [("under", at(-v)) for v in (36.0, 38.0, 745.0, 746.0, 1e9, 1e300)]
    cols += [("nonfinite", (lambda zz, v=v: v)) for v in (-INF, INF, math.nan)]
    while len(z) % 4 == 0 or len(z) % 2 == 0:
        z = z + [z[1]]
    while len(cols) % 4 == 0 or len(cols) % 2 == 0:
        cols = cols + [cols[len(cols) // 3]]
    f = np.array([[gen(zz) for _, gen in cols] for zz in z], dtype=np.float64)
    return np.array(z, dtype=np.float64), f, [r for r, _ in cols]


# ---- the truth ----------------------------------------------------------------------------------------------------------------
def gamma_form(k, t):
    """(value, derivative) at a finite real t as the header states them: mpf, or floats where e^t is above the exponential's
    range"""
    k, t = mp.mpf(k), mp.mpf(t)
    if t > HUGE or mp.exp(t) >= EXP_OVERFLOW:
        return INF, -INF
    if t < -HUGE:  # e^t = 0
        return -k * t, k
    return k * (mp.exp(t) - t), -k * mp.expm1(t)


def full_nll(k, y, mu):
    """-log Gamma(y; shape k, mean mu) from the definition: rate k / mu"""
    k, y, mu = mp.mpf(k), mp.mpf(y), mp.mpf(mu)
    return -(k * mp.log(k / mu) - mp.loggamma(k) + (k - 1) * mp.log(y) - k * y / mu)


def point_truth(pair, pset, kind, z, f):
    """(T, unit) of one fp64 point (z, f).  T is an mpf, or a float where the header states an IEEE special: a NaN in z or f
    (or z and f infinite with the same sign), +inf / -inf where t = z - f is +inf or above the exponential's range, and the
    value +inf where t is -inf (the derivative is k there: an mpf)."""
    k = PARAMS[pset]
    z, f = float(z), float(f)
    if math.isfinite(z) and math.isfinite(f):
        v, d = gamma_form(k, mp.mpf(z) - mp.mpf(f))
    else:
        t = z - f  # (IEEE: NaN, +inf or -inf)
        v, d = (math.nan, math.nan) if math.isnan(t) else (INF, -INF) if t > 0 else (INF, mp.mpf(k))
    t = v if kind == "value" else d
    return t, (math.nan if isinstance(t, float) else U * abs(t))


@functools.lru_cache(maxsize=None)
def truth(pair, pset, kind):
    """dict of (N, J) fp64 arrays: hi + lo = the truth (hi alone for specials), unit = an ulp of it"""
    z, f, _ = grid(pair, pset)
    n, j = f.shape
    hi, lo, unit = np.zeros((n, j)), np.zeros((n, j)), np.zeros((n, j))
    for a in range(n):
        for b in range(j):
            t, _ = point_truth(pair, pset, kind, float(z[a]), float(f[a, b]))
            if isinstance(t, float):
                hi[a, b], lo[a, b], unit[a, b] = t, 0.0, math.nan
                continue
            hi[a, b], lo[a, b] = T._split(t)
            unit[a, b] = T._ulp(hi[a, b])
    return {"hi": hi, "lo": lo, "unit": unit}


errors = T.errors
by_regime = T.by_regime
bound = T.bound  # the project's rule, unchanged: the larger of 4x the recorded reference error and 4 units


def cells():
    return [(pair, pset) for pair in PAIRS for pset in PARAMS]


def applies(pair, kind):
    return True


# ---- the host restatement and the library's objects ----------------------------------------------------------------------------
class GammaHostCost(O._Cost):
    """The device formulas restated plainly in fp64 torch (project code, not the reference's), in the form of the oracle's
    costs, so oracle.pls_oracle.PLS and train_pls take it unchanged.  ``z_train`` holds the logarithms of the observations.
    t = z - f is held as hi + lo (a two-sum: exact), and lo enters to first order."""

    observation_noise = None

    def __init__(self, z_train, link_function, concentration):
        assert isinstance(link_function, ExpLink)
        self.z_train, self.link_function, self.concentration = z_train, link_function, float(concentration)
        self.y_train = torch.exp(z_train)

    def _t(self, f):
        z = self.z_train[:, None].to(f.dtype).expand_as(f)
        hi = z - f
        fv = hi - z
        lo = (z - (hi - fv)) + (-f - fv)
        return hi, torch.where(hi.abs() < 1024, lo, torch.zeros_like(lo))

    def _values(self, f):
        hi, lo = self._t(f)
        e_hi = torch.exp(hi)
        v = ((e_hi + e_hi * lo) - hi) - lo
        return self.concentration * torch.where(e_hi == INF, e_hi, v)

    def calculate_cost(self, f):
        return self._values(f).sum(dim=0)

    def calculate_cost_derivative(self, f, force_autograd=False):
        hi, lo = self._t(f)
        e_hi = torch.exp(hi)
        em1 = torch.expm1(hi) + e_hi * lo
        return -self.concentration * torch.where(e_hi == INF, e_hi, em1)


def host_cost(pair, pset, z):
    return GammaHostCost(z, ExpLink(), PARAMS[pset])


def gpu_cost(P, pair, pset, z):
    return P.costs.GammaCost.from_logs(z, P.links.ExponentialLinkFunction(), PARAMS[pset])


def host_eval(pair, pset, kind, z=None, f=None):
    """the host restatement per element, (N, J): on the grid, or on the (z, f) handed in"""
    if z is None:
        z, f, _ = grid(pair, pset)
    zt, ft = torch.as_tensor(z), torch.as_tensor(f)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        if kind == "value":
            return host_cost(pair, pset, zt)._values(ft).numpy()
        return host_cost(pair, pset, zt).calculate_cost_derivative(ft, force_autograd=kind == "deriv_autograd").numpy()
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
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gamma_cost_reference_errors.json")) as fh:
        return json.load(fh)


# ---- what the family batteries take (tests/test_gpu_family_cost_{train,elements}.py) and the route tests ---------------------------
CHECKPOINT = ("concentration", 0.75)  # the attribute a checkpoint carries, and the value the model it is loaded into was built with
VALUE_TRUTH_FINITE = False  # (above the exponential's range the value is +inf)
ROUTE_PAIR = "gamma/exp"  # its own compile-time instantiation: every route, both derivative modes
ROUTE_RUNTIME_PAIR = None  # no pair of this family goes through the run-time-switch instantiation
ROUTE_SMALL_RANK_SETS = "ab"  # the parameter sets the small-rank shapes cycle through: the logarithms differ from lane to lane here
TRAIN_CONCENTRATION = 4.0


def train_y(pr, n):
    """Gamma variates of shape TRAIN_CONCENTRATION around the mean exp(fstar)"""
    g = torch.Generator().manual_seed(11 + n)
    unit = torch._standard_gamma(torch.full((n,), TRAIN_CONCENTRATION, dtype=torch.float64), generator=g) / TRAIN_CONCENTRATION
    return torch.exp(pr["fstar"].reshape(-1).double()) * unit.clamp_min(1e-300)


def train_costs(P, y, concentration=TRAIN_CONCENTRATION):
    y = y.double()
    return (GammaHostCost(torch.log(y), ExpLink(), concentration),
            P.costs.GammaCost(y, P.links.ExponentialLinkFunction(), concentration=concentration))


def check_trained_cost(gc):
    assert bool((gc.y_train > 0).all()) and torch.equal(gc.y_device().cpu(), torch.log(gc.y_train.double()))


def check_elements(got, pset):
    with np.errstate(invalid="ignore"):
        assert all(not (got["deriv_reference", strided] > PARAMS[pset]).any() for strided in (False, True)), "the derivative exceeds k"
