"""GPU: train_pls with OrdinalCost under the identity link, on both bases: the loop of tests/train_loop_fixtures.py -- 20
iterations against oracle.pls_oracle.train_pls driven by the host restatement of tests/ordinal_cost_truth.py, one launch per
iteration, and a checkpoint saved half way, loaded into a model built with other cutpoints and resumed bit for bit."""
import pytest
import torch

import ordinal_cost_truth as CT
from oracle import pls_oracle as O
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)
from train_loop_fixtures import SHAPES, training_loop

pytestmark = pytest.mark.gpu

THRESHOLDS = [-1.5, -0.25, 1.0]  # four grades cut from the noisy latent


def _y(pr, n):
    g = torch.Generator().manual_seed(11 + n)
    uniform = torch.rand(n, generator=g, dtype=torch.float64).clamp(1e-12, 1 - 1e-12)
    latent = 1.5 * pr["fstar"].reshape(-1).double() + torch.log(uniform) - torch.log1p(-uniform)  # logistic noise
    return torch.bucketize(latent, torch.tensor(THRESHOLDS, dtype=torch.float64)).double()


def _costs(P, y, cutpoints=None):
    if cutpoints is None:
        cutpoints = P.costs.OrdinalCost.cutpoints_from_labels(y, num_categories=len(THRESHOLDS) + 1)
    return CT.OrdinalHostCost(y, O.IdentityLink(), cutpoints), P.costs.OrdinalCost(y, P.links.IdentityLinkFunction(), cutpoints=cutpoints)


@pytest.mark.parametrize("base", ["onb", "ipb"])
@pytest.mark.parametrize("n,m,j", SHAPES)
def test_training_loop_against_the_host_restatement(P, route, tmp_path, n, m, j, base):  # noqa: F811
    gc = training_loop(P, route, tmp_path, n, m, j, base, _y, _costs, "cutpoints", [-3.0, 0.125, 7.0])
    assert len(set(gc.y_train.tolist())) == len(THRESHOLDS) + 1
