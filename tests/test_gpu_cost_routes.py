"""GPU: every cost epilogue per element on every route of the step.  The selector problems of tests/step_fixtures.py make G
observable through a step: a probe row k of the output is -eta 2^p G[n_k, :] without one rounding after cost_deriv, so it
must equal (torch.equal) the element-wise entry's G on the host-built F -- which tests/test_gpu_cost_elements.py holds to
the mpmath truth -- whatever the route, its tiling, its compile-time specialisation, the output form or the energy request.
All eight (cost, link) pairs and both derivative modes of Bernoulli/sigmoid, probe rows placed at the head, the middle and
the ragged tail of the data rows.  The carrier row (sum_n c_n G[n, j] plus prior) is held to its summation bound against
fsum, the energies to fsum of the mpmath cost values; the three Winograd quadrants that read S1..S4 are held per element to
4x the error of the route's own formulas run in fp64 on the host (the two rows whose left-hand operands hold the carrier:
to the summation bound of their N / 2-term products).  Gaussian/identity is the one pair whose G depends on the route: the
GEMM epilogues evaluate one fma per element, and their probe rows are held to that operation order emulated on the host."""
import numpy as np
import pytest
import torch

import cost_truth as T
from cost_families import truth_module
from step_fixtures import (EXACT_ETA, SELECTOR_PLACEMENTS, WINO_EDGES, WINO_THREE_CHUNKS, SelectorIpbProblem, SelectorProblem, option,
                           probe_winograd, run_selector_forms, spread_columns, step_wg, winograd_option, wino_one_chunk_bytes)
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks
from test_winograd_host import _winograd

pytestmark = pytest.mark.gpu

# (pair, force_autograd): the eight pairs, and Bernoulli/sigmoid's other derivative mode
VARIANTS = [(p, False) for p in T.PAIRS] + [("bernoulli/sigmoid", True)]
IDS = [p + ("/autograd" if fa else "") for p, fa in VARIANTS]


def sample(j):
    if j <= 512:
        return None
    return torch.unique(torch.cat([spread_columns(j), torch.tensor([j - 1])]))


def placement(*key):
    return SELECTOR_PLACEMENTS[sum(key) % len(SELECTOR_PLACEMENTS)]


def energy_check(P, ex, gb, cost, e, what, cols=None, gauss_fma=False, truth=False, particle_energy=True):
    """The energy by-product ``e`` and fused_particle_energy, on every route: on the sampled columns against fsum of the
    element-wise entry's cost values on the host-built F plus the exact prior (SelectorProblem.energy_direct: N roundings
    of the sum, nothing per element); ``truth``: also on three columns against fsum of the mpmath cost values, N roundings
    and per element the pair's bound of test_gpu_cost_elements (its truth module's) in the element's unit."""
    got = [("by-product", e)]
    if particle_energy:
        got.append(("fused_particle_energy", gb.fused_particle_energy(cost, ex.u.cuda(), force_generic=True)))
    idx = torch.arange(ex.j) if cols is None else torch.as_tensor(cols)
    want, tol = ex.energy_direct(P, idx, gauss_fma=gauss_fma)
    for name, en in got:
        err = (en.cpu()[idx] - want).abs()
        assert (err <= tol).all(), f"{what}: energy {name} off by {(err / tol).max().item():.2f} x its summation bound"
    if truth:
        idx = torch.unique(torch.linspace(0, ex.j - 1, 3).long())
        want, mag, units = ex.energy_truth(idx)
        tm = truth_module(ex.pair)
        b = max(tm.bound(v) for v in tm.reference_errors()[ex.pair][ex.pset]["value"].values())
        tol = (ex.n + 2) * 2.0 ** -53 * (mag + want.abs()) + b * units
        for name, en in got:
            err = (en.cpu()[idx] - want).abs()
            print(f"{what} energy {name}: max error / bound {(err / tol).max().item():.3f}")
            assert (err <= tol).all(), f"{what}: energy {name} off by {(err / tol).max().item():.2f} x its bound"


def g_direct(P, ex, cost, cols, fa):
    """the element-wise entry's G in the derivative mode ``fa``; in a family whose two modes are one formula (MODES_AGREE),
    the same bits as the other mode's"""
    g = ex.g_direct(P, cost, cols, force_autograd=fa)
    if fa and truth_module(ex.pair).MODES_AGREE:
        assert torch.equal(g, ex.g_direct(P, cost, cols, force_autograd=False)), "the two derivative modes differ"
    return g


def run(P, pair, fa, mk, n, j, place, what, force_generic=True, truth=None, setup=None, gemm=True, pset="a"):
    """``gemm``: the route's forward GEMM carries the cost in its epilogue.  For Gaussian/identity that epilogue is one fma
    per element (SelectorProblem.g_gauss_fma): the probe rows are held, bit for bit, to that operation order emulated on the
    host; every other pair runs cost_deriv itself there.  ``truth``: the energies also against mpmath (default: N <= 1600)."""
    ex = SelectorProblem(pair, mk, n, j, place, seed=mk + n + j, pset=pset)
    gb, cost = ex.basis(P), ex.cost(P, force_autograd=fa)
    if setup:
        setup(gb)
    cols = sample(j)
    g = g_direct(P, ex, cost, cols, fa)
    gauss = gemm and pair == "gaussian/identity"
    if gauss:
        g, ex.carrier_slack = ex.g_gauss_fma(g, cols)
    e = run_selector_forms(P, ex, gb, cost, g, cols, f"{what} {pair} {place}", force_generic)
    energy_check(P, ex, gb, cost, e, f"{what} {pair} {place}", cols, gauss, truth if truth is not None else n <= 1600)
    return ex, gb, cost


# every compile-time specialisation sees the first tiles' row slots and the rows from N / 2 on every GEMM route
PLACES = ("head", "half")


# -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mk,n,j,chunk", [(256, 20000, 1000, None), (256, 20000, 1000, 20000 // 3), (1024, 8000, 8192, None)])
def test_plain_general_route(P, pair, fa, mk, n, j, chunk):
    """one chunk with 16 split-K slabs, three chunks, one slab"""
    def setup(gb):
        if chunk:
            gb.workspace_bytes = P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, chunk)

    with winograd_option(P, 0):
        for place in PLACES:
            run(P, pair, fa, mk, n, j, place, f"plain chunk {chunk}", setup=setup)


@pytest.mark.parametrize("place", SELECTOR_PLACEMENTS)
@pytest.mark.parametrize("pair", ["poisson/square", "bernoulli/sigmoid"])
def test_probe_placements(P, pair, place):
    """every placement of the probe rows on one shape with N off the 128 grid: all row slots of the first tiles, the rows
    from N / 2, the ragged last tile, a spread sample with row 0 and row N - 1"""
    with winograd_option(P, 0):
        run(P, pair, False, 300, 2950, 333, place, "placements")


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mk", [129, 200, 1000])
def test_row_block_route(P, pair, fa, mk):
    n, j = 12000, 1100
    for mode in (1, 0):
        with row_blocks(P, mode):
            for place in PLACES:
                run(P, pair, fa, mk, n, j, place, f"row blocks {mode}, mk {mk}")


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mode", [2, 3])
def test_ksplit_routes(P, pair, fa, mode):
    for mk, n, j in ((200, 1500, 333), (1024, 3000, 1024)):
        with ksplit(P, mode):
            for place in PLACES:
                run(P, pair, fa, mk, n, j, place, f"k-split {mode}", truth=(n <= 1600 and place == "head"))


SMALL = [(100, 10, 64), (333, 17, 37), (3000, 30, 40), (1530, 120, 200), (900, 128, 48), (40, 12, 5)]


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("mode", [2, 0])
def test_small_rank_routes(P, pair, fa, mode):
    """M_k <= 128: the one-launch step (PLS_OPT_SMALL_RANK_STEP 2) and the slab kernels + update launch (0)"""
    for i, (n, mk, j) in enumerate(SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, mode):
            for place in (placement(len(pair), int(fa), i), placement(len(pair), int(fa), i + 2)):
                run(P, pair, fa, mk, n, j, place, f"small rank {mode} {n}x{mk}x{j}", truth=(n <= 1530 and place == "head"), gemm=False)


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_small_shapes_through_the_gemm_route(P, pair, fa):
    """PLS_OPT_SMALL_RANK_MAX 0: the same small shapes through the GEMM + epilogue route"""
    L = P.pkg._lib
    for i, (n, mk, j) in enumerate(SMALL):
        with option(P, L.OPT_SMALL_RANK_MAX, 0):
            for place in PLACES:
                run(P, pair, fa, mk, n, j, place, f"small rank off {n}x{mk}x{j}", truth=False)


# -------------------------------------------------------------------------------------------------------------------------
def _winograd_orders(a, g, slabs=16):
    """D = A G by the route's formulas in fp64 with the products summed in three orders: as the BLAS takes them, reversed,
    and in ``slabs`` split-K slabs added in turn (the device sums its products slab by slab and chunk by chunk)"""
    n = a.shape[1]
    nh = n // 2
    yield _winograd(a, g)
    flip = np.concatenate([np.arange(nh)[::-1], nh + np.arange(nh)[::-1]])
    yield _winograd(np.ascontiguousarray(a[:, flip]), np.ascontiguousarray(g[flip]))
    bounds = np.linspace(0, nh, slabs + 1).astype(int)
    tot = None
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx = np.concatenate([np.arange(lo, hi), nh + np.arange(lo, hi)])
        part = _winograd(np.ascontiguousarray(a[:, idx]), np.ascontiguousarray(g[idx]))
        tot = part if tot is None else tot + part
    yield tot


def winograd_case(P, pair, fa, mk, n, j, place, three_chunks=False, pset="a"):
    """The Winograd route: top-left quadrant as everywhere (probe rows torch.equal: out of place, strided, as new state, with
    per-block step sizes), the energies of EpiWinoCost / EpiWinoGauss against fsum, the other three per element within 4x
    the error the route's formulas make in fp64 on the host on the same G (tests/test_winograd_host.py _winograd; the
    largest over three summation orders of the products), in units of (|A11| + |A12| + |A21| + |A22|) (|G11| + |G12| + |G21|
    + |G22|) -- the sizes the seven products combine -- with a floor of 2^-52 for the roundings of the final combination."""
    ex = SelectorProblem(pair, mk, n, j, place, seed=mk + n + j, pset=pset)
    gb, cost = ex.basis(P), ex.cost(P, force_autograd=fa)
    lib = P.pkg._lib.load()
    u, xi = ex.u.cuda(), P.basis.NoiseSpec(injected=ex.injected.cuda())
    if three_chunks:
        gb.workspace_bytes = 9 * lib.pls_onb_step_workspace_bytes(gb._desc(), j, 0) // 10
        assert probe_winograd(P, gb, cost, u), "the shape does not take the Winograd route"

        def step(energy=None, eta=EXACT_ETA, **kw):
            return gb.fused_step(cost, u, eta, noise=xi, force_generic=True, input_energy=energy, **kw)
    else:  # a workspace for all paired rows in one chunk
        ws = wino_one_chunk_bytes(mk, n, j)
        planes = gb._winograd_planes(gb._desc())
        assert planes is not None and probe_winograd(P, gb, cost, u, ws_bytes=ws), "the shape does not take the Winograd route"

        def step(energy=None, eta=EXACT_ETA, **kw):
            return step_wg(P, gb, cost, u, eta, planes, noise=xi, energy=energy, ws_bytes=ws, **kw)
    first = spread_columns(j, per_tile=1)
    first = first[: len(first) // 2]
    cols = torch.cat([first, first + j // 2])
    g = ex.g_direct(P, cost, cols, force_autograd=fa)
    if pair == "gaussian/identity":  # (csrc/winograd.h EpiWinoGauss: the fma of EpiGaussDeriv, on every row)
        g, _ = ex.g_gauss_fma(g, cols, rows=torch.arange(n))
    e = torch.empty(j, device="cuda")
    got = step(e)
    assert torch.equal(got, step()), "the energy request moved the step"
    energy_check(P, ex, gb, cost, e, f"winograd {pair} {place}", cols, pair == "gaussian/identity", particle_energy=False)
    mh, ch = mk // 2, len(first)

    def top_left(out, name, **kw):
        want, probe, tol = ex.expected(g, cols, **kw)
        top = probe.clone()
        top[mh:] = False
        out = out.cpu()[:, cols]
        assert torch.equal(out[top][:, :ch], want[top][:, :ch]), f"winograd {pair} {name}: top-left probe rows differ from -eta 2^p G[n_k]"
        assert ((out[ex.k0] - want[ex.k0]).abs()[:ch] <= tol[:ch]).all(), f"winograd {pair} {name}: carrier row, top-left quadrant"
        return out, want, probe, tol

    wide = torch.full((mk, j + 64), float("nan"), device="cuda")
    step(out=wide[:, :j])
    assert torch.equal(wide[:, :j], got) and wide[:, j:].isnan().all(), f"winograd {pair}: strided output"
    del wide
    top_left(step(new_state=True), "new state", new_state=True)
    bc = 3 * j // 8  # blocks of 3/8 J straddle J / 2, the second one frozen
    etas = torch.tensor([EXACT_ETA, 0.0, 4 * EXACT_ETA])
    blocked = step(eta=0.0, blocks=P.basis.BlockSpec(bc, etas.cuda()), new_state=True)
    top_left(blocked, "blocks", eta=etas[cols // bc], new_state=True)
    assert torch.equal(blocked[:, bc:2 * bc].cpu(), ex.u[:, bc:2 * bc]), f"winograd {pair}: a frozen block moved"
    del blocked
    got, want, probe, tol = top_left(got, "out of place")
    a, gn = ex.a.numpy(), g.numpy()
    prior = EXACT_ETA * ex.u[:, cols] / ex.lam[:, None]
    hosts = [torch.as_tensor(-EXACT_ETA * d) - prior for d in _winograd_orders(a, gn)]
    nh = n // 2
    aa = np.abs(a[:mh, :nh]) + np.abs(a[:mh, nh:]) + np.abs(a[mh:, :nh]) + np.abs(a[mh:, nh:])
    gg = np.abs(gn[:nh, :ch]) + np.abs(gn[:nh, ch:]) + np.abs(gn[nh:, :ch]) + np.abs(gn[nh:, ch:])
    scale = torch.as_tensor(EXACT_ETA * (aa @ gg))
    live = scale > 0
    # the two rows whose left-hand operands hold the carrier (k0 and its partner M_k / 2 + k0) are sums of N / 2 terms in
    # every product that reads S1..S4: their error depends on the summation order, bounded as the carrier row's is
    a11, a12, a21, a22 = a[:mh, :nh], a[:mh, nh:], a[mh:, :nh], a[mh:, nh:]
    g11, g12, g21, g22 = gn[:nh, :ch], gn[:nh, ch:], gn[nh:, :ch], gn[nh:, ch:]
    s1 = a21 + a22
    s2 = s1 - a11
    t1 = g12 - g11
    t2 = g22 - t1
    pairs = ((a11, g11), (a12, g21), (a12 - s2, g22), (a22, t2 - g21), (s1, t1), (s2, t2), (a11 - a21, g22 - g12))
    rows2 = [ex.k0]
    summed = torch.as_tensor(EXACT_ETA * nh * 2.0 ** -53 * sum(np.abs(l[rows2]) @ np.abs(r) for l, r in pairs))[0]
    out = {}
    for name, rows, cs in (("top-right", slice(0, mh), slice(ch, None)), ("bottom-left", slice(mh, None), slice(0, ch)),
                           ("bottom-right", slice(mh, None), slice(ch, None))):
        slack = torch.zeros_like(scale)
        slack[ex.k0] = summed + (tol[cs] if name == "top-right" else 0.0)

        def over(x):
            return ((x[rows, cs] - want[rows, cs]).abs() - slack).clamp_min(0)

        eh = max((over(h)[live] / scale[live]).max().item() for h in hosts)
        eg = (over(got)[live] / scale[live]).max().item()
        print(f"winograd {pair} {mk}x{n}x{j} {name}: host {eh:.3e}  gpu {eg:.3e}  (units of the products' sizes)")
        out[name] = (eh, eg)
        assert (over(got)[~live] == 0).all(), f"winograd {pair} {name}: an element whose products are all zero is not"
        # away from the carrier's two rows every product has at most two nonzero terms, whose sum rounds the same in any order
        rest = torch.ones(mh, dtype=torch.bool)
        rest[ex.k0] = False
        assert torch.equal(got[rows, cs][rest], hosts[0][rows, cs][rest]), f"winograd {pair} {name}: differs from the host's formulas"
        assert eg <= max(4 * eh, 2.0 ** -52), f"winograd {pair} {name}: {eg:.3e} against the host's {eh:.3e}"
    return out


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_winograd_route(P, pair, fa):
    i = IDS.index(pair + ("/autograd" if fa else ""))
    mk, n, j = WINO_EDGES[i % len(WINO_EDGES)]
    for place in PLACES:
        winograd_case(P, pair, fa, mk, n, j, place)


@pytest.mark.parametrize("pair", ["poisson/square", "bernoulli/probit", "multimodal/identity"])
def test_winograd_three_chunks(P, pair):
    winograd_case(P, pair, False, *WINO_THREE_CHUNKS, "half", three_chunks=True)


# -------------------------------------------------------------------------------------------------------------------------
# the inducing-point basis
def run_ipb(P, pair, fa, m, n, j, place, what, chunk=None, whitened=False, truth=None, gemm=True, explicit_inverse=False, pset="a"):
    ex = SelectorIpbProblem(pair, m, n, j, place, seed=m + n + j, pset=pset)
    gb, cost = ex.basis(P, explicit_inverse=explicit_inverse), ex.cost(P, force_autograd=fa)
    if chunk:
        gb.workspace_bytes = P.pkg._lib.load().pls_ipb_step_workspace_bytes(gb._desc(), j, chunk)
    assert torch.equal(gb.whiten(ex.u.cuda()).cpu(), ex.s), "whiten"
    cols = sample(j)
    g = g_direct(P, ex, cost, cols, fa)
    gauss = gemm and pair == "gaussian/identity"
    if gauss:
        g, ex.carrier_slack = ex.g_gauss_fma(g, cols)
    e = run_selector_forms(P, ex.whitened(whitened), gb, cost, g, cols, f"{what} {pair} {place}", whitened=whitened)
    energy_check(P, ex, gb, cost, e, f"{what} {pair} {place}", cols, gauss, truth if truth is not None else n <= 1600)


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
@pytest.mark.parametrize("m,n,j,chunk", [(200, 300, 333, None), (200, 20000, 333, None), (200, 20000, 333, 20000 // 3),
                                         (1024, 8000, 512, None)])
def test_ipb_general_route(P, pair, fa, m, n, j, chunk):
    """solve, the drift streamed over row chunks (one; three) and split-K slabs (N = 300: one; N = 20000: several), update"""
    for place in PLACES:
        run_ipb(P, pair, fa, m, n, j, place, f"ipb general chunk {chunk}", chunk=chunk, truth=(n <= 1600 and place == "head"))


IPB_SMALL = [(100, 10, 64), (333, 17, 37), (1000, 32, 100), (1100, 128, 90), (520, 65, 16)]  # (N, M, J)


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_ipb_one_launch_route(P, pair, fa):
    """at most 128 inducing points: the one-launch step behind the one-launch solve"""
    for i, (n, m, j) in enumerate(IPB_SMALL):
        with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, 2):
            for place in (placement(len(pair), int(fa), i), "tail"):
                run_ipb(P, pair, fa, m, n, j, place, f"ipb one launch {n}x{m}x{j}", gemm=False, truth=(place == "tail" and n <= 1000))


@pytest.mark.parametrize("pair,fa", VARIANTS, ids=IDS)
def test_ipb_whitened_entries(P, pair, fa):
    """Whitened coordinates.  For a cost other than Gaussian/identity the basis has one whitened step: the one-launch step on
    the operand Awa, k(X,Z) Lc^-T stacked on sqrt(M) Lc^-T (M a power of four).  Its last rows are the prior's
    (csrc/small_rank_step.h); the probe on data row N - 1 ("tail") sits next to them."""
    for n, m, j in ((100, 4, 64), (333, 16, 37), (1000, 64, 100)):
        for place in ("tail", "head"):
            run_ipb(P, pair, fa, m, n, j, place, f"ipb whitened generic {n}x{m}x{j}", whitened=True, truth=False, gemm=False)
