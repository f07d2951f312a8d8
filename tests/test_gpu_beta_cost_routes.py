"""GPU: the Beta/sigmoid epilogue per element on every route of the step, as tests/test_gpu_family_cost_routes.py holds the
negative binomial: a probe row of a selector problem is -eta 2^p G[n_k, :] without one rounding after cost_deriv, so it must
equal (torch.equal) the element-wise entry's G on the host-built F -- which tests/test_gpu_family_cost_elements.py holds to the
mpmath truth -- whatever the route, its tiling, its compile-time specialisation, the output form or the energy request.  The
carrier row is held to its summation bound against fsum, the energies to fsum of the element-wise values and, on the small
shapes, of the mpmath values.  Beta/probit, the chain rule through the run-time-switch instantiation, runs the plain route
and the small-rank route.  Shapes: the smallest at which each route can still go wrong."""
import pytest

import beta_cost_truth as CT
import test_gpu_cost_routes as R
from step_fixtures import option, winograd_option
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks

pytestmark = pytest.mark.gpu

BETA = CT.ROUTE_PAIR
# (pair, force_autograd): both derivative modes of the dedicated pair (the same bits, through the same instantiation)
VARIANTS = [(BETA, False), (BETA, True)]
IDS = [BETA, BETA + "/autograd"]
RUNTIME = CT.ROUTE_RUNTIME_PAIR


# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,fa", VARIANTS + [(RUNTIME, False)], ids=IDS + [RUNTIME])
@pytest.mark.parametrize("chunks", [1, 3])
def test_plain_general_route(P, pair, fa, chunks):
    """N off the 128 grid, M_k and J off the tile: one chunk, and three chunks through a smaller workspace"""
    mk, n, j = 300, 2950, 333

    def setup(gb):
        if chunks > 1:
            gb.workspace_bytes = P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, -(-n // chunks))

    with winograd_option(P, 0):
        for place in R.PLACES:
            R.run(P, pair, fa, mk, n, j, place, f"plain, {chunks} chunk(s)", setup=setup, truth=False)


def test_second_parameter_set_on_the_plain_route(P):
    with winograd_option(P, 0):
        R.run(P, BETA, False, 300, 2950, 333, "tail", "plain, phi = 400", truth=False, pset="b")


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mk,mode", [(129, 1), (200, 0)])
def test_row_block_route(P, pair, fa, mk, mode):
    with row_blocks(P, mode):
        for place in R.PLACES:
            R.run(P, pair, fa, mk, 3000, 520, place, f"row blocks {mode}, mk {mk}")


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mode", [2, 3])
def test_ksplit_routes(P, pair, fa, mode):
    with ksplit(P, mode):
        for place in R.PLACES:
            R.run(P, pair, fa, 200, 1500, 333, place, f"k-split {mode}", truth=(place == "head"))


@pytest.mark.parametrize("pair,fa", VARIANTS + [(RUNTIME, False)], ids=IDS + [RUNTIME])
@pytest.mark.parametrize("mode", [2, 0])
def test_small_rank_routes(P, pair, fa, mode):
    """M_k <= 128: the one-launch step (PLS_OPT_SMALL_RANK_STEP 2) and the slab kernels + update launch (0)"""
    for i, (n, mk, j) in enumerate(R.SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, mode):
            for place in (R.placement(len(pair), int(fa), i), R.placement(len(pair), int(fa), i + 2)):
                R.run(P, pair, fa, mk, n, j, place, f"small rank {mode} {n}x{mk}x{j}", truth=(n <= 1530 and place == "head" and i < 2))


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_small_shapes_through_the_gemm_route(P, pair, fa):
    """PLS_OPT_SMALL_RANK_MAX 0: two of the small shapes through the GEMM + epilogue route"""
    L = P.pkg._lib
    for n, mk, j in (R.SMALL[1], R.SMALL[3]):
        with option(P, L.OPT_SMALL_RANK_MAX, 0):
            for place in R.PLACES:
                R.run(P, pair, fa, mk, n, j, place, f"small rank off {n}x{mk}x{j}", truth=False)


def test_winograd_route(P):
    R.winograd_case(P, BETA, False, 512, 16384, 2048, "half")


# -------------------------------------------------------------------------------------------------------------------------
# the inducing-point basis
@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_ipb_general_route(P, pair, fa):
    for place in R.PLACES:
        R.run_ipb(P, pair, fa, 200, 300, 333, place, "ipb general", truth=(place == "head"))


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_ipb_one_launch_route(P, pair, fa):
    for i, (n, m, j) in enumerate(R.IPB_SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, 2):
            for place in (R.placement(len(pair), int(fa), i), "tail"):
                R.run_ipb(P, pair, fa, m, n, j, place, f"ipb one launch {n}x{m}x{j}", truth=(place == "tail" and n <= 333))


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_ipb_whitened_entries(P, pair, fa):
    for n, m, j in ((100, 4, 64), (333, 16, 37)):
        for place in ("tail", "head"):
            R.run_ipb(P, pair, fa, m, n, j, place, f"ipb whitened generic {n}x{m}x{j}", whitened=True, truth=False)
