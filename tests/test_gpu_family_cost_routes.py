"""GPU: the epilogue of every family's dedicated pair (tests/cost_families.py; Beta and Gamma in files of their own,
tests/test_gpu_{beta,gamma}_cost_routes.py) per element on every route of the step, as
tests/test_gpu_cost_routes.py holds the reference's pairs: a probe row of a selector problem is -eta 2^p G[n_k, :] without one
rounding after cost_deriv, so it must equal (torch.equal) the element-wise entry's G on the host-built F -- which
tests/test_gpu_family_cost_elements.py holds to the mpmath truth -- whatever the route, its tiling, its compile-time
specialisation, the output form or the energy request.  The carrier row is held to its summation bound against fsum, the
energies to fsum of the element-wise values and, on the small shapes, of the mpmath values.  The truth module names the pairs:
ROUTE_PAIR, with a compile-time instantiation of its own, runs every route in both derivative modes (the same bits, through the
same instantiation); ROUTE_RUNTIME_PAIR, where a family has one, runs the plain route and the small-rank routes -- Gaussian/exp,
the exponential link through the run-time-switch instantiation.  Shapes: the smallest at which each route can still go wrong,
the same for every family.  (The tests/test_<family>_cost_host.py files hold the selector problems themselves to their regimes.)"""
import pytest

import test_gpu_cost_routes as R
from cost_families import FAMILIES, family_name, truth_module
from step_fixtures import option, winograd_option
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks

pytestmark = pytest.mark.gpu
HERE = [CT for CT in FAMILIES if family_name(CT) not in ("beta", "gamma")]  # (those two: test_gpu_{beta,gamma}_cost_routes.py)


def _variants(runtime):
    """(pair, force_autograd) of every family, its name first in the id: both derivative modes of the dedicated pair and, on
    the routes that ask for it, the run-time-switch pair of the families that have one"""
    out = []
    for CT in HERE:
        pairs = [(CT.ROUTE_PAIR, False), (CT.ROUTE_PAIR, True)]
        if runtime and CT.ROUTE_RUNTIME_PAIR:
            pairs.append((CT.ROUTE_RUNTIME_PAIR, False))
        out += [pytest.param(pair, fa, id=f"{family_name(CT)}-{pair}" + "/autograd" * fa) for pair, fa in pairs]
    return out


VARIANTS = _variants(runtime=False)
WITH_RUNTIME = _variants(runtime=True)
DEDICATED = [pytest.param(CT.ROUTE_PAIR, id=family_name(CT)) for CT in HERE]


# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("pair,fa", WITH_RUNTIME)
def test_plain_general_route(P, pair, fa, chunks):
    """N off the 128 grid, M_k and J off the tile: one chunk, and three chunks through a smaller workspace"""
    mk, n, j = 300, 2950, 333

    def setup(gb):
        if chunks > 1:
            gb.workspace_bytes = P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, -(-n // chunks))

    with winograd_option(P, 0):
        for place in R.PLACES:
            R.run(P, pair, fa, mk, n, j, place, f"plain, {chunks} chunk(s)", setup=setup, truth=False)


@pytest.mark.parametrize("pair", DEDICATED)
def test_second_parameter_set_on_the_plain_route(P, pair):
    with winograd_option(P, 0):
        R.run(P, pair, False, 300, 2950, 333, "tail", "plain, set b", truth=False, pset="b")


@pytest.mark.parametrize("mk,mode", [(129, 1), (200, 0)])
@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_row_block_route(P, pair, fa, mk, mode):
    with row_blocks(P, mode):
        for place in R.PLACES:
            R.run(P, pair, fa, mk, 3000, 520, place, f"row blocks {mode}, mk {mk}")


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_ksplit_routes(P, pair, fa, mode):
    with ksplit(P, mode):
        for place in R.PLACES:
            R.run(P, pair, fa, 200, 1500, 333, place, f"k-split {mode}", truth=(place == "head"))


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("pair,fa", WITH_RUNTIME)
def test_small_rank_routes(P, pair, fa, mode):
    """M_k <= 128: the one-launch step (PLS_OPT_SMALL_RANK_STEP 2) and the slab kernels + update launch (0); the shapes cycle
    through the family's ROUTE_SMALL_RANK_SETS"""
    sets = truth_module(pair).ROUTE_SMALL_RANK_SETS
    for i, (n, mk, j) in enumerate(R.SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, mode):
            for place in (R.placement(len(pair), int(fa), i), R.placement(len(pair), int(fa), i + 2)):
                R.run(P, pair, fa, mk, n, j, place, f"small rank {mode} {n}x{mk}x{j}", truth=(n <= 1530 and place == "head" and i < 2),
                    pset=sets[i % len(sets)])


@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_small_shapes_through_the_gemm_route(P, pair, fa):
    """PLS_OPT_SMALL_RANK_MAX 0: two of the small shapes through the GEMM + epilogue route"""
    L = P.pkg._lib
    for n, mk, j in (R.SMALL[1], R.SMALL[3]):
        with option(P, L.OPT_SMALL_RANK_MAX, 0):
            for place in R.PLACES:
                R.run(P, pair, fa, mk, n, j, place, f"small rank off {n}x{mk}x{j}", truth=False)


@pytest.mark.parametrize("pair", DEDICATED)
def test_winograd_route(P, pair):
    """at the route's eligibility floor"""
    R.winograd_case(P, pair, False, 512, 16384, 2048, "half")


# -------------------------------------------------------------------------------------------------------------------------
# the inducing-point basis
@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_ipb_general_route(P, pair, fa):
    for place in R.PLACES:
        R.run_ipb(P, pair, fa, 200, 300, 333, place, "ipb general", truth=(place == "head"))


@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_ipb_one_launch_route(P, pair, fa):
    for i, (n, m, j) in enumerate(R.IPB_SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, 2):
            for place in (R.placement(len(pair), int(fa), i), "tail"):
                R.run_ipb(P, pair, fa, m, n, j, place, f"ipb one launch {n}x{m}x{j}", truth=(place == "tail" and n <= 333))


@pytest.mark.parametrize("pair,fa", VARIANTS)
def test_ipb_whitened_entries(P, pair, fa):
    for n, m, j in ((100, 4, 64), (333, 16, 37)):
        for place in ("tail", "head"):
            R.run_ipb(P, pair, fa, m, n, j, place, f"ipb whitened generic {n}x{m}x{j}", whitened=True, truth=False)
