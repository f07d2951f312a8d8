"""GPU: train_pls with the cost of every family (tests/cost_families.py) under its dedicated link, on both bases: the loop of
tests/train_loop_fixtures.py -- 20 iterations against oracle.pls_oracle.train_pls driven by the host restatement of the
family's truth module, one launch per iteration, and a checkpoint saved half way, loaded into a model built with another value
of the cost's parameter (CHECKPOINT), whose parameter travels with the particles, and resumed bit for bit.  The truth module
states how y is drawn (train_y), how the two costs are built from it (train_costs) and what the family asserts on the cost that
trained (check_trained_cost)."""
import pytest

from cost_families import FAMILIES, family_name
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_small_step import route  # noqa: F401  (fixture)
from train_loop_fixtures import SHAPES, training_loop

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("base", ["onb", "ipb"])
@pytest.mark.parametrize("n,m,j", SHAPES)
@pytest.mark.parametrize("CT", [pytest.param(CT, id=family_name(CT)) for CT in FAMILIES])
def test_training_loop_against_the_host_restatement(P, route, tmp_path, CT, n, m, j, base):  # noqa: F811
    CT.check_trained_cost(training_loop(P, route, tmp_path, n, m, j, base, CT.train_y, CT.train_costs, *CT.CHECKPOINT))
