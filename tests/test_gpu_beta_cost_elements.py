"""GPU: what the Beta pairs test of their own next to tests/test_gpu_family_cost_elements.py, which holds the element-wise
entries to the per-element mpmath truth of tests/beta_cost_truth.py on its whole grid (bulk, the centre and the root where the
derivative cancels, both tails, the far columns where exp(-|f|) underflows while value and derivative stay finite, +-0 and
subnormals; beta/probit on both sides of the clip): the two examples of the far tails, and the device special functions
themselves (pls_debug_math ops 4-6) per element against mpmath.

The bound is tests/test_gpu_cost_elements.py's, unchanged: per cell the larger of 4x the host restatement's recorded error
(tests/golden/beta_cost_reference_errors.json) and 4 units.  PLS_COST_TRUTH_DUMP=<file> appends the measured maxima as JSON
lines (the rows of DESIGN.md section 3 are made from them)."""
import math

import pytest
import torch

import beta_cost_truth as BT
import test_gpu_cost_elements as E
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def test_the_tails_stay_finite_and_the_drift_is_exactly_one(P):
    """the issue's two examples: the value at f = 745, phi = 0.3 (lgamma(phi exp(-745)) itself is +inf), and the derivative at
    f = +-1e300, exactly +-1 for any phi and z"""
    z = torch.tensor([0.0], dtype=torch.float64)
    v = BT.gpu_cost(P, "beta/sigmoid", "a", z).calculate_cost(torch.tensor([[745.0]], device="cuda")).item()
    assert math.isfinite(v) and abs(v - 747.3) < 0.05
    for pset in BT.PARAMS:
        cost = BT.gpu_cost(P, "beta/sigmoid", pset, torch.tensor(BT.Z_ROWS))
        f = torch.tensor([[1e300, -1e300, 1e10, -1e10]], device="cuda").repeat(len(BT.Z_ROWS), 1)
        d = cost.calculate_cost_derivative(f).cpu()
        assert torch.equal(d[:, :2], torch.tensor([[1.0, -1.0]]).repeat(len(BT.Z_ROWS), 1).double())
        assert torch.equal(d[:, 2:], d[:, :2])


@pytest.mark.parametrize("name", list(BT.SPECIALS))
def test_special_functions_against_mpmath(P, name):
    """pls_debug_math ops 4-6 per element: log-spaced over the fp64 range, across the seams of the pieces, and dense around 1,
    the zero of psi and 2"""
    x, regimes = BT.special_points(name)
    xt = torch.as_tensor(x).cuda()
    out = torch.empty_like(xt)
    lib = P.pkg._lib.load()
    P.pkg._lib.check(lib.pls_debug_math(BT.SPECIALS[name], xt.data_ptr(), out.data_ptr(), xt.numel(), None), "pls_debug_math")
    torch.cuda.synchronize()
    err = BT.special_by_regime(BT.errors(out.cpu().numpy().reshape(-1, 1), BT.special_truth(name)), regimes)
    rec = BT.reference_errors()["special"][name]
    missed = []
    for regime, v in err.items():
        bound = BT.bound(rec[regime])
        print(f"{name:9s} {regime:10s} gpu {v:10.3g}  host {rec[regime]!s:>10}  bound {bound:.3g}")
        E._dump({"pair": "special", "pset": name, "kind": "value", "regime": regime, "gpu": v if math.isfinite(v) else "inf", "oracle": rec[regime]})
        if not v <= bound:
            missed.append((regime, v, bound))
    assert not missed, f"{name}: regimes over their bound (regime, error, bound): {missed}"
    # X(0) = -1 exactly (no pole), and lgamma's exact zeros
    probe = torch.tensor([0.0, 1.0, 2.0], device="cuda")
    res = torch.empty_like(probe)
    P.pkg._lib.check(lib.pls_debug_math(BT.SPECIALS[name], probe.data_ptr(), res.data_ptr(), 3, None), "pls_debug_math")
    res = res.cpu()
    if name == "xdigamma":
        assert res[0].item() == -1.0
    if name == "lgamma":
        assert res[0].item() == math.inf and res[1].item() == 0.0 and res[2].item() == 0.0
