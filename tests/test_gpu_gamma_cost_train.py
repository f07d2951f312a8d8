"""GPU: train_pls with GammaCost under the exponential link, on both bases: the loop of tests/train_loop_fixtures.py -- 20
iterations against oracle.pls_oracle.train_pls driven by the host restatement of tests/gamma_cost_truth.py, one launch per
iteration, and a checkpoint saved half way, loaded into a model built with another concentration and resumed bit for bit."""
import pytest
import torch

import gamma_cost_truth as CT
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)
from train_loop_fixtures import SHAPES, training_loop

pytestmark = pytest.mark.gpu

CONCENTRATION = 4.0


def _y(pr, n):
    """Gamma variates of shape CONCENTRATION around the mean exp(fstar)"""
    g = torch.Generator().manual_seed(11 + n)
    unit = torch._standard_gamma(torch.full((n,), CONCENTRATION, dtype=torch.float64), generator=g) / CONCENTRATION
    return torch.exp(pr["fstar"].reshape(-1).double()) * unit.clamp_min(1e-300)


def _costs(P, y, concentration=CONCENTRATION):
    y = y.double()
    return (CT.GammaHostCost(torch.log(y), CT.ExpLink(), concentration),
            P.costs.GammaCost(y, P.links.ExponentialLinkFunction(), concentration=concentration))


@pytest.mark.parametrize("base", ["onb", "ipb"])
@pytest.mark.parametrize("n,m,j", SHAPES)
def test_training_loop_against_the_host_restatement(P, route, tmp_path, n, m, j, base):  # noqa: F811
    gc = training_loop(P, route, tmp_path, n, m, j, base, _y, _costs, "concentration", 0.75)
    assert bool((gc.y_train > 0).all()) and torch.equal(gc.y_device().cpu(), torch.log(gc.y_train.double()))
