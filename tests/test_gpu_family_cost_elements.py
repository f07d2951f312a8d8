"""GPU: the element-wise entries for the pairs of every cost family (tests/cost_families.py) -- pls_cost_derivative (both
derivative modes, which must be the same bits) and pls_cost_value -- against the per-element mpmath truth of the family's truth
module on its whole grid, dense and strided, and the column sums of the values.  What only one family tests -- its edges, its
special functions, its link entry -- stays in tests/test_gpu_{count,beta,ordinal,gamma}_cost_elements.py.

The bound is tests/test_gpu_cost_elements.py's, unchanged: per (pair, parameter set, kind, regime) the larger of 4x the host
restatement's recorded error (tests/golden/<family>_cost_reference_errors.json) and 4 units; IEEE specials must match exactly.
PLS_COST_TRUTH_DUMP=<file> appends the measured maxima as JSON lines (the rows of DESIGN.md section 3 are made from them)."""
import numpy as np
import pytest

import test_gpu_cost_elements as E
from cost_families import FAMILIES, family_name
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CELLS = [pytest.param(CT, pair, pset, id=f"{family_name(CT)}-{pair}-{pset}") for CT in FAMILIES for pair, pset in CT.cells()]


@pytest.mark.parametrize("CT,pair,pset", CELLS)
def test_elements_against_truth(P, CT, pair, pset):
    got = E.elements_against_truth(P, CT, pair, pset)
    if CT.MODES_AGREE:
        E.modes_agree(got)
    if CT.check_elements:
        CT.check_elements(got, pset)


@pytest.mark.parametrize("CT,pair,pset", CELLS)
def test_value_column_sums(P, CT, pair, pset):
    if CT.VALUE_TRUTH_FINITE:
        assert np.isfinite(CT.truth(pair, pset, "value")["hi"]).all()
    E.value_column_sums(P, CT, pair, pset)
