"""GPU: what the count-model pairs test of their own next to tests/test_gpu_family_cost_elements.py, which holds the element-wise
entries to the per-element mpmath truth of tests/count_cost_truth.py on its whole grid (bulk, the root where the derivative
cancels, both tails, the far columns where e^f leaves the fp64 range while the negative binomial stays finite, +-0 and
subnormals): predict_samples through the link entry pls_link_transform, and the negative binomial under the square link."""
import math

import pytest
import torch

import count_cost_truth as CT
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_predict_samples_with_a_column_offset(P):
    """predict_samples = exp(f + eps_j) in one kernel: against the link entry on the host-formed sum (the same bits), and
    against the truth of the link at that sum"""
    y, f, regimes = CT.grid("negative_binomial/exp", "a")
    cost = CT.gpu_cost(P, "negative_binomial/exp", "a", torch.as_tensor(y))
    g = torch.Generator().manual_seed(5)
    eps = torch.randn(f.shape[1], generator=g, dtype=torch.float64)
    ft = torch.as_tensor(f)
    got = cost.predict_samples(ft.cuda(), observation_noise=eps.cuda()).cpu()
    shifted = ft + eps[None, :]
    assert torch.equal(got, cost.link_function(shifted.cuda()).cpu())
    fin = shifted.abs() < 700
    want = torch.tensor([[float(mp_exp(v)) for v in row] for row in shifted.tolist()], dtype=torch.float64)
    assert ((got - want).abs()[fin] <= 4 * 2.0 ** -52 * want[fin]).all()
    assert (got[shifted > 710] == math.inf).all() and (got[shifted < -746] == 0).all()
    assert cost.sample_observation_noise(7).abs().sum() == 0  # observation_noise is None: no draw, as for Poisson


def test_negative_binomial_under_another_link(P):
    """The square link: the header's formula in mu = f^2 by the generic chain rule (run-time-switch code only), in the bulk,
    against mpmath.  Units: 2^-53 x the sizes of the two terms of value and derivative; bound 16 -- two log1p of a
    two-piece sum (each: a division or a product by 1 / r, the logarithm), two products and the sum for the value, one
    division of products and the slope for the derivative, every primitive <= 1 ulp."""
    import mpmath as mp

    y = torch.tensor([0.0, 1.0, 3.0, 25.0, 1e6, 0.5, 1.0 / 3.0], dtype=torch.float64)
    f = torch.tensor([0.3, -0.3, 0.9, -0.9, 1.3, -1.3, 2.6, -2.6, 2.95, -2.95, 17.0], dtype=torch.float64).repeat(len(y), 1)
    for r in (0.7, 50.0):
        cost = P.costs.NegativeBinomialCost(y, P.links.SquareLinkFunction(), r)
        d = cost.calculate_cost_derivative(f.cuda()).cpu()
        assert torch.equal(d, cost.calculate_cost_derivative(f.cuda(), force_autograd=True).cpu())
        for a in range(len(y)):
            v = P.costs.NegativeBinomialCost(y[a:a + 1], P.links.SquareLinkFunction(), r).calculate_cost(f[a:a + 1].cuda()).cpu()
            for b in range(f.shape[1]):
                rr, yy, ff = mp.mpf(r), mp.mpf(float(y[a])), mp.mpf(float(f[a, b]))
                mu = ff * ff
                t1, t2 = rr * mp.log1p(mu / rr), yy * mp.log1p(rr / mu)
                assert abs(mp.mpf(float(v[b])) - (t1 + t2)) <= 16 * CT.U * (abs(t1) + abs(t2)), (r, a, b, float(v[b]), t1 + t2)
                g1, g2 = rr * mu / (mu * (rr + mu)) * 2 * ff, rr * yy / (mu * (rr + mu)) * 2 * ff
                assert abs(mp.mpf(float(d[a, b])) - (g1 - g2)) <= 16 * CT.U * (abs(g1) + abs(g2)), (r, a, b, float(d[a, b]), g1 - g2)


def mp_exp(v):
    import mpmath as mp

    return mp.exp(mp.mpf(v)) if abs(v) < 1e4 else (mp.inf if v > 0 else mp.mpf(0))
