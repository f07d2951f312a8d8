"""GPU: what the Gamma cost tests of its own next to tests/test_gpu_family_cost_elements.py, which holds the element-wise
entries to the per-element mpmath truth of tests/gamma_cost_truth.py on its whole grid (bulk, the root down to a subnormal
difference, the rounded subtraction at |t| in the hundreds, the overflow edge, the underflow side and a non-finite f): the
edges include/plship.h tables, also for the non-finite z the grid cannot hold, and the derivative's relative accuracy at its
root."""
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import gamma_cost_truth as CT
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PAIR = "gamma/exp"
INF = math.inf


def _raw(P, pset, z):
    """the cost on logarithms from_logs would refuse: they are handed to the library as they are"""
    cost = CT.gpu_cost(P, PAIR, pset, torch.zeros(len(z), dtype=torch.float64))
    cost._z_dev = torch.tensor(z, dtype=torch.float64).cuda()
    return cost


@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_the_edges_of_the_header(P, pset):
    """the table of include/plship.h per element, one (z, f) per row -- t = +inf and above the exponential's range: +inf and
    -inf, never NaN; e^t underflowed: -k t and exactly k; z = -inf or f = +inf: +inf and k; a NaN: NaN (and for z and f
    infinite with the same sign); a finite row between them keeps its values"""
    k = CT.PARAMS[pset]
    pts = [(INF, 0.3), (INF, -1e300), (INF, -INF), (-INF, 0.3), (-INF, 1e300), (-INF, INF), (math.nan, 0.3), (math.nan, INF),
           (0.3, math.nan), (INF, INF), (-INF, -INF), (INF, math.nan), (0.3, -INF), (0.3, INF), (0.3, 0.3 - 709.79), (0.3, 0.3 - 1e6),
           (1e308, -1e308), (-8e307, 8e307), (0.3, 1e300), (0.3, 746.3), (0.3, 38.3), (0.3, 0.3), (0.3, -0.9)]
    cost = _raw(P, pset, [p[0] for p in pts])
    f = torch.tensor([[p[1]] for p in pts], dtype=torch.float64).cuda()
    g = cost.calculate_cost_derivative(f).cpu().numpy()[:, 0]
    g_auto = cost.calculate_cost_derivative(f, force_autograd=True).cpu().numpy()[:, 0]
    assert np.array_equal(g, g_auto, equal_nan=True), "the two derivative modes differ"
    v = np.array([_raw(P, pset, [zz]).calculate_cost(torch.tensor([[ff]], dtype=torch.float64).cuda()).item() for zz, ff in pts])
    for a, (zz, ff) in enumerate(pts):
        for kind, got in (("value", v[a]), ("deriv_reference", g[a])):
            t = CT.point_truth(PAIR, pset, kind, zz, ff)[0]
            if not math.isfinite(float(t)):  # (a stated special, or a finite truth beyond the fp64 range: -k t at t = -1.6e308, k = 2.5)
                assert (math.isnan(float(t)) and math.isnan(got)) or got == float(t), (kind, zz, ff, got, t)
            else:
                assert abs(mp.mpf(float(got)) - t) <= 4 * CT.U * abs(t), (kind, zz, ff, got, t)
    named = dict(zip(pts, zip(v, g)))
    assert named[(INF, 0.3)] == (INF, -INF) and named[(0.3, -INF)] == (INF, -INF) and named[(1e308, -1e308)] == (INF, -INF)
    assert named[(-INF, 0.3)] == (INF, k) and named[(0.3, INF)] == (INF, k) and named[(-8e307, 8e307)][1] == k
    assert named[(0.3, 746.3)][1] == k and named[(0.3, 38.3)][1] == k and named[(0.3, 1e300)] == (k * 1e300, k)
    assert named[(0.3, 0.3)] == (k, 0.0)
    assert np.isnan(_raw(P, pset, [p[0] for p in pts]).calculate_cost(f.expand(-1, 3).contiguous()).cpu().numpy()).all()  # (a NaN row poisons every sum)


@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_the_derivative_is_relatively_accurate_at_its_root(P, pset):
    """f = z + d for d from one ulp of z up to 2^-20, both signs, on every row of the grid: the derivative is -k expm1(-d),
    within 4 x 2^-53 of itself -- not of k, which is what 1 - e^t would leave"""
    z = np.array(CT.Z_ROWS[:6])
    steps = np.array([s * 2.0 ** -e for e in range(20, 53, 4) for s in (1, -1)])
    f = z[:, None] * (1 + steps[None, :])
    got = CT.gpu_cost(P, PAIR, pset, torch.as_tensor(z)).calculate_cost_derivative(torch.as_tensor(f).cuda()).cpu().numpy()
    for a in range(len(z)):
        for b in range(len(steps)):
            want = CT.point_truth(PAIR, pset, "deriv_reference", z[a], f[a, b])[0]
            assert want != 0 and abs(mp.mpf(float(got[a, b])) - want) <= 4 * CT.U * abs(want), (z[a], f[a, b], got[a, b], want)
