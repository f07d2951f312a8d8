"""GPU: what the ordinal cost tests of its own next to tests/test_gpu_family_cost_elements.py, which holds the element-wise
entries to the per-element mpmath truth of tests/ordinal_cost_truth.py on its whole grid (bulk, both sides of every cutpoint,
the root of an interior label where the derivative cancels, both tails, the far columns where the value is linear or
underflows gradually, +-0 and subnormals): what the header states for a y that is not a category index (NaN) and for a label
past the last category (+inf and -1), and the exact zeros and ends of the edge labels."""
import math

import numpy as np
import pytest
import torch

import ordinal_cost_truth as CT
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _raw(P, pset, labels):
    """the cost on labels its constructor would refuse: they are handed to the library as they are"""
    cost = CT.gpu_cost(P, "ordinal/identity", pset, torch.zeros(len(labels), dtype=torch.float64))
    cost.y_train = torch.tensor(labels, dtype=torch.float64)
    return cost


@pytest.mark.parametrize("pset", list(CT.PARAMS))
def test_a_y_that_is_no_category_index_gives_nan(P, pset):
    """one row each of y = 2.5, -1, 5 and NaN (and a valid row between them, which keeps its values)"""
    f = torch.tensor([[-40.0, -1.0, -0.0, 0.3, 2.0, 700.0, 1e300]], dtype=torch.float64).repeat(5, 1).cuda()
    labels = [2.5, -1.0, 1.0, 5.0, math.nan]
    g = _raw(P, pset, labels).calculate_cost_derivative(f).cpu()
    g_auto = _raw(P, pset, labels).calculate_cost_derivative(f, force_autograd=True).cpu()
    assert np.array_equal(g.numpy(), g_auto.numpy(), equal_nan=True), "the two derivative modes differ"
    assert torch.isnan(g[[0, 1, 3, 4]]).all() and torch.isfinite(g[2]).all()
    assert torch.equal(g[2], CT.gpu_cost(P, "ordinal/identity", pset, torch.ones(1)).calculate_cost_derivative(f[2:3]).cpu()[0])
    for a, yy in enumerate(labels):
        v = _raw(P, pset, [yy]).calculate_cost(f[a:a + 1]).cpu()
        assert torch.isnan(v).all() if a != 2 else torch.isfinite(v).all(), (yy, v)
    assert torch.isnan(_raw(P, pset, labels).calculate_cost(f).cpu()).all()  # (a NaN row poisons every column sum)


def test_a_label_past_the_last_category_gives_inf_and_minus_one(P):
    """set b has three categories: the lower cutpoint of labels 3 and 4 is +inf -- value +inf, derivative -1, whatever f"""
    f = torch.tensor([[-1e300, -40.0, -0.0, 0.3, 700.0, 1e300]], dtype=torch.float64).repeat(2, 1).cuda()
    cost = _raw(P, "b", [3.0, 4.0])
    assert (cost.calculate_cost_derivative(f).cpu() == -1).all()
    assert (cost.calculate_cost(f).cpu() == math.inf).all()


def test_edge_terms_are_exactly_zero_and_the_ends_exact(P):
    """the bottom category's lower and the top category's upper term are exactly 0: far on its own side an edge label costs
    exactly 0 with derivative 0, and far on the other side exactly |f - b| with derivative +-1"""
    f = torch.tensor([[-1e300, -1e10, 1e10, 1e300]], dtype=torch.float64).repeat(2, 1).cuda()
    cost = CT.gpu_cost(P, "ordinal/identity", "a", torch.tensor([0.0, 4.0], dtype=torch.float64))
    g = cost.calculate_cost_derivative(f).cpu()
    assert torch.equal(g, torch.tensor([[0.0, 0.0, 1.0, 1.0], [-1.0, -1.0, 0.0, 0.0]], dtype=torch.float64))
    lo = CT.gpu_cost(P, "ordinal/identity", "a", torch.zeros(1)).calculate_cost(f[:1]).cpu()
    hi = CT.gpu_cost(P, "ordinal/identity", "a", torch.full((1,), 4.0)).calculate_cost(f[1:]).cpu()
    assert torch.equal(lo, torch.tensor([0.0, 0.0, 1e10 + 1.5, 1e300], dtype=torch.float64))
    assert torch.equal(hi, torch.tensor([1e300, 1e10 + 2.0, 0.0, 0.0], dtype=torch.float64))
