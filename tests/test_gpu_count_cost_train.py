"""GPU: train_pls with NegativeBinomialCost under the exponential link, on both bases: the loop of
tests/train_loop_fixtures.py -- 20 iterations against oracle.pls_oracle.train_pls driven by the host restatement of
tests/count_cost_truth.py, one launch per iteration, and a checkpoint saved half way, whose dispersion travels with the
particles, resumed bit for bit."""
import pytest
import torch

import count_cost_truth as CT
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)
from train_loop_fixtures import SHAPES, training_loop

pytestmark = pytest.mark.gpu

R_DISPERSION = 3.0


def _y(pr, n):
    """over-dispersed counts around exp(1 + f*): a gamma-mixed Poisson with shape r"""
    rate = torch.exp(1.0 + pr["fstar"])
    mix = torch.distributions.Gamma(torch.tensor(R_DISPERSION, dtype=torch.float64), torch.tensor(R_DISPERSION, dtype=torch.float64))
    torch.manual_seed(11 + n)
    return torch.poisson(rate * mix.sample((n,)))


def _costs(P, y, dispersion=R_DISPERSION):
    return (CT.NegativeBinomialHostCost(y, CT.ExpLink(), dispersion),
            P.costs.NegativeBinomialCost(y, P.links.ExponentialLinkFunction(), dispersion))


@pytest.mark.parametrize("base", ["onb", "ipb"])
@pytest.mark.parametrize("n,m,j", SHAPES)
def test_training_loop_against_the_oracle(P, route, tmp_path, n, m, j, base):  # noqa: F811
    gc = training_loop(P, route, tmp_path, n, m, j, base, _y, _costs, "dispersion", 99.0)
    assert gc.dispersion == R_DISPERSION
