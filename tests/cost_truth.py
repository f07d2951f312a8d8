"""A per-element truth for the eight (cost, link) pairs: cost(y, f), d cost / d f in both derivative modes and the link
itself, written in mpmath (50 digits) as the reference defines them (link_functions.py, costs/*.py, restated by
oracle/pls_oracle.py) -- the clip to [jitter, 1 - jitter] with slope 0 outside it, the Bernoulli/sigmoid closed form on the
CLIPPED p, multimodal's autograd value -- on a grid of (y, f) organised in named regimes, and the error units the tests
measure in.

Inputs are fp64 numbers taken exactly; constants (pi, sqrt 2) are mathematical; ``1 - jitter`` is the fp64 number the
reference's clip uses.  A truth beyond the fp64 range is +-inf; the specials of the reference's own arithmetic at the Poisson
pole f = +-0 (0 * inf, inf * sgn(0)) are stated, not computed.

Error units.  Every regime is measured in ulps of the truth, except the regimes whose formula cancels; those use
2^-53 x (|T| + the absolute values of the cancelling terms, carried to the result):

  regime                unit     cancelling terms
  root (Poisson)        cancel   value: |2 y log|f|| + p; derivative: |2 y / f| + |slope|
  root (Gaussian/sq.)   cancel   f^2 against y: |dT/dp| f^2
  Bernoulli, all but    cancel   1 - p (rounds at the size of 1 + p whichever clip is near, and when p is clipped):
  bulk and zero                  |dT/d(1-p)| (1 + p); probit's 1 + erf: |dT/dp| (1 + |erf|) / 2 (sigmoid: |dT/dp| p);
                                 the derivative's two terms, which cancel where p is near a non-binary y (p_near_y)
  tie (multimodal)      cancel   the two exponents' terms: (1 + A) x sum |terms|, A = |l1| + |l2| + (e1^2 + e2^2) / (2 s2)
  Student-t's value     cancel   log(1 + x), x = e^2 / (nu s^2), loses x's bits below 1's: (nu + 1) / 2
  everything else       ulp

Two of the reference's own artefacts are kept as grid points and measured, not followed: its autograd returns NaN for the
sigmoid where exp(-f) overflows (regime "overflow"; the slope outside the clip is 0), and torch's logsumexp backward does not
normalise its weights once the exponents absorb the log-weights (regime "absorbed").

(dT/dp: the sensitivity of the result to the link value, taken numerically in mpmath; 0 where p is clipped, since the clip
bounds are exact.)"""
import functools
import math

import mpmath as mp
import numpy as np
import torch

from oracle import pls_oracle as O

mp.mp.dps = 50
PAIRS = ["gaussian/identity", "poisson/square", "bernoulli/sigmoid", "bernoulli/probit", "student_t/identity",
         "multimodal/identity", "poisson/identity", "gaussian/square"]
KINDS = ["value", "deriv_reference", "deriv_autograd", "link"]
# parameter sets: "a" = step_fixtures.oracle_costs / make_costs; "b" = a second set per cost (Poisson has no parameters)
PARAMS = {
    "a": {"gaussian": (0.3,), "student_t": (3.0, 0.7), "multimodal": (0.7, 1.5, 0.3), "jitter": 1e-10},
    "b": {"gaussian": (2.5,), "student_t": (5.5, 1.3), "multimodal": (0.4, -2.0, 0.65), "jitter": 1e-6},
}
CANCEL = {"root", "tie"}
BERNOULLI_CANCEL = {"lo_tail", "hi_tail", "clip_lo", "clip_hi", "clipped", "overflow", "p_near_y"}
CLIP_MARGIN = 2.0 ** -44
ORACLE_MISS = 1e6  # units beyond which a recorded oracle error is a miss of the oracle, not a rounding
U = mp.mpf(2) ** -53
# What the selector problems of tests/step_fixtures.py take from a family (every truth module states these three):
# |f| of the grid values that may carry a selector problem (on top of finite and >= 1e-30): here any up to 1e30, whose
# products with |c_n| <= 8 stay finite
SELECTOR_RANGE = {pair: (lambda a: a <= 1e30) for pair in PAIRS}
OWN_CARRIER_STREAM = False  # the carrier values and labels come from the problem's one generator, with everything else
MODES_AGREE = False  # the two derivative modes are different formulas (Bernoulli/sigmoid: closed form against autograd)


def unit_kind(pair, kind, regime):
    cost, link = pair.split("/")
    if regime in CANCEL or (cost == "bernoulli" and regime in BERNOULLI_CANCEL):
        return "cancel"
    if cost == "student_t" and kind == "value":
        return "cancel"
    return "ulp"


# ---- the grid -----------------------------------------------------------------------------------------------------------------
def _raw(link, f):
    f = mp.mpf(f)
    if link == "sigmoid":
        return 1 / (1 + mp.exp(-f))
    return (1 + mp.erf(f / mp.sqrt(2))) / 2


def _inv_link(link, raw):
    if link == "sigmoid":
        return mp.log(raw / (1 - raw))
    # probit: solve (1 + erf(f / sqrt 2)) / 2 = raw through the complementary function (no cancellation in either tail)
    if raw < 0.5:
        return -_inv_link(link, 1 - raw)
    q = 1 - raw
    x0 = mp.sqrt(-2 * mp.log(q)) if q < 0.2 else mp.mpf(0.5)
    return mp.findroot(lambda x: mp.log(mp.erfc(x / mp.sqrt(2)) / 2) - mp.log(q), x0)


def _clip_points(link, jitter):
    """f on both sides of each clip bound, the link value at relative distances 2^-20 .. 2^-40 of the bound from it"""
    lo, hi = [], []
    for bound, out in ((mp.mpf(jitter), lo), (mp.mpf(1.0 - jitter), hi)):
        # (probit's 1 + erf resolves its lower tail to 2^-53 ABSOLUTE: nearer than 2^-53 / jitter, relative, fp64 cannot tell
        # the side, and such a point would not be a test of anything)
        near = link == "probit" and bound < 0.5
        for k in ((6, 8, 10, 12, 14) if near and jitter < 1e-8 else (20, 22, 24, 26, 28) if near else (20, 24, 30, 36, 40)):
            for s in (1, -1):
                raw = bound * (1 + s * mp.mpf(2) ** -k)
                if 0 < raw < 1 and abs(1 - raw) > mp.mpf(2) ** -48:
                    out.append(float(_inv_link(link, raw)))
    return lo, hi


def _bernoulli_columns(link, jitter):
    edge = float(-_inv_link(link, mp.mpf(jitter)))  # |f| at the clips: 23.03 / 6.36 for jitter 1e-10
    lo, hi = _clip_points(link, jitter)
    cols = [("bulk", v) for v in (0.1, -0.1, 0.7, -0.7, 1.5, -1.5, 2.9, -2.9)]
    near = {"sigmoid": lambda t: math.log(t / (1 - t)), "probit": lambda t: float(_inv_link("probit", mp.mpf(t)))}[link]
    cols += [("p_near_y", v) for v in (2.0 ** -30, -1e-9, near(0.25) * (1 + 2.0 ** -30), near(0.9) * (1 - 2.0 ** -20))]
    inner = [3.0, 3.7, 0.5 * (3 + edge), 0.8 * edge, 0.95 * edge, 0.995 * edge]
    cols += [("hi_tail", v) for v in inner] + [("lo_tail", -v) for v in inner]
    cols += [("clip_lo", v) for v in lo] + [("clip_hi", v) for v in hi]
    far = [1.05 * edge, 30.0, 40.0, 100.0, 709.5] + ([745.0, 1e10, 1e150] if link == "probit" else [])
    cols += [("clipped", s * v) for v in far for s in (1, -1)]
    if link == "sigmoid":  # exp(-f) overflows (f = -745) or underflows to a subnormal (f = 745)
        cols += [("overflow", v) for v in (-745.0, 745.0, -710.0)]
    cols += [("zero", v) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.2250738585072014e-308)]
    return cols


@functools.lru_cache(maxsize=None)
def grid(pair, pset):
    """(y (N,), f (N, J), regimes (J names)): every row has its own y, a column is one regime; N and J are off every
    multiple of 4 (and so of 64)."""
    cost, link = pair.split("/")
    prm = PARAMS[pset]
    third = 1.0 / 3.0
    if cost == "bernoulli":
        y = [0.0, 1.0, 1.0, 0.0, 0.25, 1.0, 0.0, 0.0, 0.5, 1.0, 0.9, 0.0, 1.0, 1e-3, 1.0, 0.0, 1.0, 1.0, third]
        cols = [(r, (lambda yy, v=v: v)) for r, v in _bernoulli_columns(link, prm["jitter"])]
    elif cost == "poisson":
        y = [0.0, 1.0, 3.0, 1e6, 2.0, 0.0, 7.0, 1.0, 10.0, 1e6, 0.0, 4.0, 25.0, 1.0, 5.0]
        root = (lambda yy: math.sqrt(yy)) if link == "square" else (lambda yy: 2.0 * yy)
        cols = [("bulk", (lambda yy, v=v: v)) for v in (0.3, -0.3, 0.9, -0.9, 1.3, -1.3, 2.6, -2.6, 2.95, -2.95)]
        cols += [("pole", (lambda yy, v=v, s=s: s * v)) for v in (1e-300, 1e-200, 1e-100, 1e-30, 1e-10, 1e-3) for s in (1, -1)]
        cols += [("root", (lambda yy, k=k, s=s, t=t: t * root(yy) * (1 + s * 2.0 ** -k) if yy > 0 else t * 2.0 ** -k))
                 for k in (8, 20, 30, 40, 50, 60) for s in (1, -1) for t in (1, -1)]
        cols += [("tail", (lambda yy, v=v, s=s: s * v)) for v in (1e3, 1e10, 1e100, 1e150, 1e160) for s in (1, -1)]
        cols += [("zero", (lambda yy, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, -2.2250738585072014e-308)]
    elif cost == "multimodal":
        sig, shift, bn = prm["multimodal"]
        y = [0.0, 1.0, -1.0, 0.37, -2.5, 3.0, 1e-3, -0.6, 2.2, 10.0, -7.0, 0.5, third, -1.7, 5.5]
        # the modes tie where l1 - e1^2 / (2 s2) = l2 - e2^2 / (2 s2), e1 = e2 + shift
        e_tie = float((mp.log(mp.mpf(bn)) - mp.log(1 - mp.mpf(bn))) * mp.mpf(sig) ** 2 / mp.mpf(shift) - mp.mpf(shift) / 2)
        cols = [("bulk", (lambda yy, v=v: yy - v)) for v in (0.0, 0.2, -0.2, 0.9, -0.9, 1.7, -1.7, 2.5, -2.5, 0.01)]
        cols += [("tie", (lambda yy, k=k, s=s: yy - e_tie * (1 + s * 2.0 ** -k))) for k in (2, 6, 10, 20, 30, 40, 52) for s in (1, -1)]
        cols += [("underflow", (lambda yy, v=v, s=s: yy - s * v)) for v in (8.0, 30.0, 50.0, 100.0, 1e5) for s in (1, -1)]
        cols += [("absorbed", (lambda yy, v=v, s=s: yy - s * v)) for v in (1e100, 1e150) for s in (1, -1)]
        cols += [("zero", (lambda yy, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310)]
    elif pair == "gaussian/square":
        y = [0.0, 1.0, 0.3, 2.0, 1e-3, 7.5, 0.25, 4.0, 1e6, 0.0, 9.0, third, 1.21, 100.0, 0.5]
        cols = [("bulk", (lambda yy, v=v: v)) for v in (0.1, -0.1, 0.8, -0.8, 1.4, -1.4, 2.2, -2.2, 2.9, -2.9)]
        cols += [("root", (lambda yy, k=k, s=s, t=t: t * math.sqrt(yy) * (1 + s * 2.0 ** -k) if yy > 0 else t * 2.0 ** -k))
                 for k in (8, 20, 30, 40, 50) for s in (1, -1) for t in (1, -1)]
        cols += [("tail", (lambda yy, v=v, s=s: s * v)) for v in (1e3, 1e10, 1e50, 1e75, 1e100, 1e150) for s in (1, -1)]
        cols += [("zero", (lambda yy, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310, 1e-160, -1e-160)]
    else:  # gaussian/identity, student_t/identity: the error e = f - y decides the regime
        y = [0.0, 1.0, -1.0, 0.37, -2.5, 3.0, 1e-3, -0.6, 2.2, 1e6, -7.0, 0.5, third, -1.7, 5.5]
        cols = [("bulk", (lambda yy, v=v: yy + v)) for v in (0.1, -0.1, 0.8, -0.8, 1.4, -1.4, 2.2, -2.2, 2.9, -2.9)]
        cols += [("e_small", (lambda yy, v=v, s=s: yy + s * v if yy != 0 else s * v))
                 for v in (1e-3, 1e-5, 1e-8, 2.0 ** -40, 1e-100, 1e-160, 1e-200) for s in (1, -1)]
        cols += [("e_large", (lambda yy, v=v, s=s: yy + s * v)) for v in (30.0, 1e3, 1e8, 1e10, 1e100, 1e150) for s in (1, -1)]
        cols += [("zero", (lambda yy, v=v: v)) for v in (0.0, -0.0, 5e-324, -5e-324, 1e-310)]
    while len(y) % 4 == 0 or len(y) % 2 == 0:
        y = y + [y[1]]
    while len(cols) % 4 == 0 or len(cols) % 2 == 0:
        cols = cols + [cols[len(cols) // 3]]
    f = np.array([[gen(yy) for _, gen in cols] for yy in y], dtype=np.float64)
    return np.array(y, dtype=np.float64), f, [r for r, _ in cols]


# ---- the truth ----------------------------------------------------------------------------------------------------------------
def link_truth(link, f, jitter):
    """(raw, p, slope, clipped, S): the unclipped and clipped link value, d p / d f as autograd sees it (0 outside the clip),
    and S, the sum of the absolute values of the terms p is formed from where those cancel (else p's own size)"""
    f = mp.mpf(f)
    if link == "identity":
        return f, f, mp.mpf(1), False, mp.mpf(0)
    if link == "square":
        return f * f, f * f, 2 * f, False, f * f
    lo, hi = mp.mpf(jitter), mp.mpf(1.0 - jitter)
    if link == "sigmoid":
        raw = 1 / (1 + mp.exp(-f))
        slope, s = raw * (1 - raw), raw
    else:
        erf = mp.erf(f / mp.sqrt(2))
        raw = (1 + erf) / 2
        slope, s = mp.exp(-f * f / 2) / mp.sqrt(2 * mp.pi), (1 + abs(erf)) / 2
    if raw < lo or raw > hi:
        return raw, (lo if raw < lo else hi), mp.mpf(0), True, mp.mpf(0)
    return raw, raw, slope, False, s


def _from_p(cost, link, kind, prm, y, f, p, slope, q=None):
    """(T, extra): the result as a function of the link value (and, for Bernoulli, of q = 1 - p taken as a variable of its
    own), and the cancelling terms that do not pass through p"""
    zero = mp.mpf(0)
    q = 1 - p if q is None else q
    if kind == "link":
        return p, zero
    ref = kind == "deriv_reference"
    if cost == "gaussian":
        (s2,) = prm["gaussian"]
        e = p - y
        return (e * e / (2 * mp.mpf(s2)), zero) if kind == "value" else (e / mp.mpf(s2) * slope, zero)
    if cost == "poisson":
        if kind == "value":
            t = -2 * y * mp.log(abs(f))
            return t + p, abs(t) + abs(p)
        return -2 * y / f + slope, abs(2 * y / f) + abs(slope)
    if cost == "bernoulli":
        if kind == "value":
            return -mp.log(p) * y - mp.log(q) * (1 - y), zero
        if ref and link == "sigmoid":
            return -y * q + (1 - y) * p, abs(y * q) + abs((1 - y) * p)
        return (-y / p + (1 - y) / q) * slope, (abs(y / p) + abs((1 - y) / q)) * abs(slope)
    if cost == "student_t":
        nu, sc = (mp.mpf(v) for v in prm["student_t"])
        e = p - y
        if kind == "value":
            return (nu + 1) / 2 * mp.log(1 + e * e / (nu * sc * sc)), (nu + 1) / 2
        return (nu + 1) * e / (nu * sc * sc + e * e) * slope, zero
    sig, shift, bn = (mp.mpf(v) for v in prm["multimodal"])
    s2 = sig * sig
    e1, e2 = y - p + shift, y - p
    l1, l2, norm = mp.log(bn), mp.log(1 - bn), mp.log(mp.sqrt(2 * mp.pi * s2))
    a1, a2 = l1 - e1 * e1 / (2 * s2) - norm, l2 - e2 * e2 / (2 * s2) - norm
    m = max(a1, a2)
    w1, w2 = mp.exp(a1 - m), mp.exp(a2 - m)
    amp = 1 + abs(l1) + abs(l2) + (e1 * e1 + e2 * e2) / (2 * s2)
    if kind == "value":
        lse = mp.log(w1 + w2)
        return -(m + lse), amp * (abs(l1) + abs(l2) + (e1 * e1 + e2 * e2) / (2 * s2) + abs(norm) + abs(lse))
    return -(w1 * e1 + w2 * e2) / (w1 + w2) / s2 * slope, amp * (w1 * abs(e1) + w2 * abs(e2)) / (w1 + w2) / s2 * abs(slope)


def point_truth(pair, pset, kind, y, f):
    """(T, cancel unit) of one fp64 point; T is an mpf, or a float special (+-inf / nan) stated from the reference's
    arithmetic at the Poisson pole"""
    cost, link = pair.split("/")
    prm = PARAMS[pset]
    if cost == "poisson" and f == 0.0 and kind != "link":
        if kind == "value":  # -2 y log 0 + 0: +inf, or 0 * -inf
            return (math.inf if y > 0 else math.nan), None
        # the closed form of the square link divides by f; autograd (and any other link) multiplies 1 / |f| by sgn(0) = 0
        if kind == "deriv_reference" and link == "square" and y > 0:
            return -math.copysign(math.inf, f), None
        return math.nan, None
    raw, p, slope, clipped, s = link_truth(link, f, prm["jitter"])
    ym, fm = mp.mpf(y), mp.mpf(f)
    t, extra = _from_p(cost, link, kind, prm, ym, fm, p, slope)
    sens = mp.mpf(0)
    if not clipped and s != 0:
        d = p * mp.mpf(2) ** -100
        sens = abs(_from_p(cost, link, kind, prm, ym, fm, p + d, slope, 1 - p)[0] - t) / d
    sens_q = mp.mpf(0)
    if cost == "bernoulli" and kind != "link":  # forming 1 - p rounds at the size of 1 + p, clipped or not
        d = mp.mpf(2) ** -120
        sens_q = abs(_from_p(cost, link, kind, prm, ym, fm, p, slope, 1 - p + d)[0] - t) / d
    return t, U * (abs(t) + sens * s + sens_q * (1 + p) + extra)


def _split(t):
    """an mpf as hi + lo in fp64 (inf beyond the range)"""
    hi = float(t)
    if not math.isfinite(hi):
        return hi, 0.0
    return hi, float(t - mp.mpf(hi))


def _ulp(x):
    x = abs(x)
    if not math.isfinite(x):
        return math.nan
    return max(math.ulp(x), 2.0 ** -1074) if x >= 2.0 ** -1022 else 2.0 ** -1074


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
            hi[a, b], lo[a, b] = _split(t)
            unit[a, b] = float(cu) if unit_kind(pair, kind, regimes[b]) == "cancel" else _ulp(hi[a, b])
            if unit_kind(pair, kind, regimes[b]) == "cancel":
                unit[a, b] = max(unit[a, b], 2.0 ** -1074)
    return {"hi": hi, "lo": lo, "unit": unit}


def errors(got, tr):
    """per element: |got - truth| / unit; 0 where both are the same IEEE special, inf where only one is special or the
    specials differ"""
    got = np.asarray(got, dtype=np.float64)
    hi, lo, unit = tr["hi"], tr["lo"], tr["unit"]
    special = ~np.isfinite(hi)
    same = (np.isnan(hi) & np.isnan(got)) | (np.isinf(hi) & (got == hi))
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs((got - hi) - lo) / unit
    err = np.where(special, np.where(same, 0.0, np.inf), err)
    return np.where(~special & ~np.isfinite(got), np.inf, err)


def by_regime(err, regimes):
    out = {}
    for b, r in enumerate(regimes):
        out[r] = max(out.get(r, 0.0), float(err[:, b].max()))
    return out


def clip_distances(pair, pset):
    """mpmath: every point's unclipped link value, as its relative distance from the nearer clip bound, and as that
    distance in units of 2^-53 x the terms fp64 forms the value from (its resolution there)"""
    cost, link = pair.split("/")
    if link not in ("sigmoid", "probit"):
        return np.zeros(0), np.zeros(0)
    jit = PARAMS[pset]["jitter"]
    _, f, _ = grid(pair, pset)
    lo, hi = mp.mpf(jit), mp.mpf(1.0 - jit)
    rel, res = [], []
    for v in np.unique(f):
        raw, _, _, _, _ = link_truth(link, v, 0.0)
        s = raw if link == "sigmoid" else (1 + abs(mp.erf(mp.mpf(v) / mp.sqrt(2)))) / 2
        rel.append(float(min(abs(raw - lo) / lo, abs(raw - hi) / hi)))
        res.append(float(min(abs(raw - lo), abs(raw - hi)) / (U * s)))
    return np.array(rel), np.array(res)


# ---- the two implementations under measurement --------------------------------------------------------------------------------
def applies(pair, kind):
    """multimodal has one derivative (always autograd); every other pair has both modes"""
    return not (pair == "multimodal/identity" and kind == "deriv_reference")


def _make(costs, links, pair, pset, y):
    cost, link = pair.split("/")
    prm = PARAMS[pset]
    lk = {"identity": lambda: links[0](), "square": lambda: links[1](), "sigmoid": lambda: links[2](prm["jitter"]),
          "probit": lambda: links[3](prm["jitter"])}[link]()
    if cost == "gaussian":
        return costs[0](prm["gaussian"][0], y, lk)
    if cost == "poisson":
        return costs[1](y, lk)
    if cost == "bernoulli":
        return costs[2](y, lk)
    if cost == "student_t":
        return costs[3](prm["student_t"][0], y, lk, prm["student_t"][1])
    return costs[4](*prm["multimodal"], y, lk)


def host_cost(pair, pset, y):
    return _make((O.GaussianCost, O.PoissonCost, O.BernoulliCost, O.StudentTCost, O.MultiModalCost),
                 (O.IdentityLink, O.SquareLink, O.SigmoidLink, O.ProbitLink), pair, pset, y)


def gpu_cost(P, pair, pset, y):
    C, Lk = P.costs, P.links
    return _make((C.GaussianCost, C.PoissonCost, C.BernoulliCost, C.StudentTCost, C.MultiModalCost),
                 (Lk.IdentityLinkFunction, Lk.SquareLinkFunction, Lk.SigmoidLinkFunction, Lk.ProbitLinkFunction), pair, pset, y)


def oracle_eval(pair, pset, kind):
    """the oracle (fp64 torch on the host) on the grid, per element: (N, J)"""
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


def measure_oracle():
    """{pair: {parameter set: {kind: {regime: the oracle's largest error in the regime's unit}}}}"""
    out = {}
    for pair in PAIRS:
        for pset in PARAMS:
            if pair.startswith("poisson") and pset != "a":
                continue
            regimes = grid(pair, pset)[2]
            for kind in KINDS:
                if applies(pair, kind):
                    err = errors(oracle_eval(pair, pset, kind), truth(pair, pset, kind))
                    out.setdefault(pair, {}).setdefault(pset, {})[kind] = by_regime(err, regimes)
    return out


def cells():
    return [(pair, pset) for pair in PAIRS for pset in PARAMS if not (pair.startswith("poisson") and pset != "a")]


# ---- the recorded oracle errors and the bound they set ------------------------------------------------------------------------
def reference_errors():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cost_truth_oracle_errors.json")) as fh:
        return json.load(fh)


def bound(recorded):
    """What an implementation built from <= 1 ulp primitives may reach in a cell: 4x the oracle's recorded maximum, or 4
    units, whichever is larger (the primitives replace libm calls that are themselves <= 1 ulp, and the formulas chain at
    most four of them).  A cell the oracle itself misses ("inf": a special the truth does not have; more than ORACLE_MISS
    units: a wrong value, as where torch's logsumexp backward stops normalising) gets the 4 units."""
    if recorded == "inf" or float(recorded) > ORACLE_MISS:
        return 4.0
    return max(4.0 * float(recorded), 4.0)
