"""GPU: every route of the orthonormal basis' step on exact problems (step_fixtures.ExactProblem): integer operands,
power-of-two eigenvalues, variance and step size, on which every route computes the step without a single rounding.  The
result must equal plain fp64 torch on the host bit for bit (torch.equal), so a dropped, doubled or misplaced contribution
of any size -- in any tile, split-K slab, chunk or Winograd product -- fails, whatever the summation order.  Routes: the
plain general route (one chunk, several chunks, one and several slabs), the Strassen-Winograd route, the row-block
back-projection, the k-split contractions of narrow J, the one-launch small-rank step and its slab kernels, the Gaussian
fast path; output out of place, into a strided buffer and as the new state; per-block step sizes with a frozen block.  The
energy by-product is compared per particle at 1e-13."""
import pytest
import torch

from step_fixtures import (EXACT_ETA, ExactProblem, assert_exact, option, probe_winograd, run_forms, spread_columns, step_wg,
                           winograd_option, wino_one_chunk_bytes)
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks

pytestmark = pytest.mark.gpu


def sample(j):
    """all columns of a narrow J; else both ends of every 128-column tile, a few in between, their J/2 partners, the last"""
    if j <= 512:
        return None
    return torch.unique(torch.cat([spread_columns(j), torch.tensor([j - 1])]))


# -------------------------------------------------------------------------------------------------------------------------
# the plain general route: one chunk with 16 split-K slabs, three chunks, one slab (512 output tiles, N <= 16384)
@pytest.mark.parametrize("mk,n,j,chunk,slabs", [(256, 20000, 1000, None, ">1"), (256, 20000, 1000, 20000 // 3, ">1"),
                                                (1024, 8000, 8192, None, "1")])
def test_plain_general_route(P, mk, n, j, chunk, slabs):
    ex = ExactProblem(mk, n, j, seed=mk + n + j)
    gb, cost = ex.basis(P), ex.cost(P)
    if chunk:
        gb.workspace_bytes = P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, chunk)
    with winograd_option(P, 0):
        run_forms(P, ex, gb, cost, sample(j), f"plain {mk}x{n}x{j} chunk {chunk}")


def test_winograd_route(P):
    """fused_step's own workspace at N = 40000: the route in two chunks of paired rows, several slabs"""
    ex = ExactProblem(512, 40000, 2048, seed=3)
    gb, cost = ex.basis(P), ex.cost(P)
    assert probe_winograd(P, gb, cost, ex.u.cuda())
    run_forms(P, ex, gb, cost, sample(2048), "winograd")


@pytest.mark.parametrize("mk", [129, 200, 300, 1000])
def test_row_block_route(P, mk):
    """ranks off the 128 grid (PLS_OPT_ROW_BLOCKS 1: one launch of equal-height tiles; 0: 128-row tiles + remainders), J off
    the 128-column grid"""
    n, j = 12000, 1100
    ex = ExactProblem(mk, n, j, seed=mk)
    gb, cost = ex.basis(P), ex.cost(P)
    u, xi = ex.u.cuda(), P.basis.NoiseSpec(injected=ex.xi.cuda())
    cols = sample(j)
    for mode in (1, 0):
        with row_blocks(P, mode):
            e = torch.empty(j, device="cuda")
            got = gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=True, input_energy=e)
            assert_exact(ex, got, cols, energy=e, what=f"row blocks {mode}, mk {mk}")
    with row_blocks(P, 1):
        run_forms(P, ex, gb, cost, cols, f"row blocks, mk {mk}")


@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("mk,n,j", [(200, 1500, 333), (1024, 3000, 1024)])
def test_ksplit_routes(P, mode, mk, n, j):
    """PLS_OPT_KSPLIT_MODE 2 / 3 forces the two- / one-group k-split kernel on narrow J: the fast path's B U and the general
    route's contractions"""
    ex = ExactProblem(mk, n, j, seed=mk + mode)
    gb, cost = ex.basis(P), ex.cost(P)
    with ksplit(P, mode):
        run_forms(P, ex, gb, cost, sample(j), f"k-split {mode} fast path", force_generic=False)
        run_forms(P, ex, gb, cost, sample(j), f"k-split {mode} general", force_generic=True)


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("n,mk,j", [(100, 10, 64), (333, 17, 37), (3000, 30, 40), (1530, 120, 200), (900, 128, 48), (40, 12, 5)])
def test_small_rank_routes(P, mode, n, mk, j):
    """M_k <= 128: the one-launch step (PLS_OPT_SMALL_RANK_STEP 2) and the slab kernels + update launch (0)"""
    ex = ExactProblem(mk, n, j, seed=n + mk)
    gb, cost = ex.basis(P), ex.cost(P)
    with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, mode):
        run_forms(P, ex, gb, cost, None, f"small rank {mode}")


@pytest.mark.parametrize("mk,n,j", [(512, 40000, 2048), (100, 3000, 333), (129, 5000, 1100)])
def test_gaussian_fast_path(P, mk, n, j):
    ex = ExactProblem(mk, n, j, seed=n + j)
    gb, cost = ex.basis(P), ex.cost(P)
    run_forms(P, ex, gb, cost, sample(j), "fast path", force_generic=False)


# -------------------------------------------------------------------------------------------------------------------------
def test_headline_shape(P):
    """N = 1e5, M_k = 1024, J = 8192: the plain and the Winograd route in the bench's 8 GiB workspace (Winograd: two chunks,
    four slabs) and the Winograd route with all paired rows in one chunk, and the fast path -- all rows, on 64 column pairs
    that hold both ends of every 128-column tile"""
    mk, n, j = 1024, 100_000, 8192
    ex = ExactProblem(mk, n, j, seed=7)
    gb, cost = ex.basis(P), ex.cost(P)
    gb.workspace_bytes = 8 << 30
    u, xi = ex.u.cuda(), P.basis.NoiseSpec(injected=ex.xi.cuda())
    cols = spread_columns(j, per_tile=0)
    assert len(cols) == 128
    want, e_want = ex.step(cols)
    assert probe_winograd(P, gb, cost, u)
    e = torch.empty(j, device="cuda")
    got = gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=True, input_energy=e)
    assert_exact(ex, got, cols, energy=e, what="winograd, 8 GiB")
    with winograd_option(P, 0):
        got = gb.fused_step(cost, u, EXACT_ETA, noise=xi, force_generic=True)
    assert_exact(ex, got, cols, what="plain, 8 GiB")
    del got
    ws = wino_one_chunk_bytes(mk, n, j)
    planes = gb._winograd_planes(gb._desc())
    assert probe_winograd(P, gb, cost, u, ws_bytes=ws)
    got = step_wg(P, gb, cost, u, EXACT_ETA, planes, noise=xi, ws_bytes=ws)
    assert_exact(ex, got, cols, what="winograd, all rows")
    got = gb.fused_step(cost, u, EXACT_ETA, noise=xi)
    assert_exact(ex, got, cols, what="fast path")
