"""GPU: the noise the step routes draw inside their kernels (csrc/philox.h normal_pair), element by element.

1.  pls_normal_fill against the 50-digit truth of the stream (tests/philox_truth.py, tests/golden/philox_truth.npz): every
    fixture entry within 9 units of 2^-53 |truth|, no absolute floor.  The bar is the sum of what the parts state for themselves,
    each in relative units at the worst position of its binade: the logarithm <= 2 ulp = 4 units, halved by the square root (2);
    sqrt_normal <= 1 ulp (2); the angle, one fma rounding and the rounding of pi / 4 * 2^-50 at a sensitivity <= 1 on [0, pi / 4]
    (2); fdlibm's kernels < 1 ulp (2); the final product (1).  Bulk blocks, the extremes one 8 x 1 fill each, a padded leading
    dimension behind NaN guards and row counts whose last pairs have no upper row.
2.  Every route that draws: the same step once with NoiseSpec(seed, step, j_offset) and once with NoiseSpec(injected = the
    pls_normal_fill block of the same counters) must agree bit for bit (torch.equal) -- injected and drawn deviates enter the same
    arithmetic --, and the step without noise must differ from both.  Inputs: the exact problems of tests/step_fixtures.py
    (their drift is exact, every difference comes from the noise), eta = EXACT_ETA, M_k = 133 where a GEMM route takes it (the
    last pair, rows 128 | 132, has a lone lower row).  Counters: (1, 0, 0); high words in seed and step with a column offset;
    j_offset = 2^32 - 3, where the column counter wraps (the stream is defined on its low 32 bits).

    Two routes cannot be bit-equal, and are held to the forward-error bound of the product that differs:
      * ipb_prep_kernel colours its own draws, E = Lc Xi, on 16 x 16 x 4 MFMA tiles; the injected E comes from pls_tri_multiply,
        another summation order.  On problems with U = 0 and y = 0 the step's output IS sqrt(2 eta) E without one more rounding
        (sqrt(2 eta) = 2^-10), so |drawn - injected| <= (M + 2) 2^-53 (|Lc| |Xi|) sqrt(2 eta) per element: each side errs by
        at most gamma_K |Lc| |Xi| with K <= M / 2 + 1 non-zeros per row of the constructed factor.
      * pls_ipb_step's two-launch Gaussian route draws white xi into dS and multiplies Lc (dS + sqrt(2 eta) xi); injected, it adds
        sqrt(2 eta) e behind the product Lc dS.  Per element |drawn - injected| <= (M + 3) 2^-53 |Lc| (|dS| + sqrt(2 eta) |Xi|)
        + 2^-53 |out|: (K + 1) roundings on the drawn side (the sum dS + sqrt(2 eta) xi, the product), K of Lc Xi and of Lc dS and
        the final sum on the injected side.
    A misplaced draw differs by O(sqrt(2 eta)) ~ 1e-3, more than ten orders above either bound.

The seven call sites of normal_pair on step routes, and the parametrisations that reach them.  The launches' timeline tags
(asserted in each test) tell the kernel families apart; inside "gemm_langevin_gaussian" the tiling follows pick_gemm_cfg
(csrc/plship.hip) from PLS_OPT_KSPLIT_MODE and the count of 128 x 128 tiles, inside "langevin_update" probe_winograd tells the
Winograd update from the plain one:

  EpiLangevinGaussian, 128 x 128 direct epilogue   test_gaussian_fast_path_tilings[0-16400] (2 x 129 tiles: interior tiles of tile
                                                   row 0; tile row 1 and the last tile column take the LDS epilogue at 128 x 128)
  EpiLangevinGaussian, 64 x 64 LDS epilogue        test_gaussian_fast_path_tilings[0-333], [0-1100] (below 256 tiles), [3-*] (one
                                                   k-group), test_ipb_whitened_step, test_ipb_two_launch_gaussian_step
  EpiLangevinGaussian, k-split draw before k-loop  test_gaussian_fast_path_tilings[1-*] (auto), [2-*] (two k-groups)
  langevin_update_kernel                           test_plain_general_route, test_row_block_route, test_small_rank_routes[0-*],
                                                   test_ipb_general_route (its draws coloured by a separate launch)
  langevin_update_wino_kernel                      test_winograd_route
  one-launch small-rank step (small_rank_step.h)   test_small_rank_routes[2-*], test_ipb_whitened_generic_step
  ipb_prep_kernel                                  test_ipb_prep_colours_the_streams_draws

Measured on the MI355X (profiles/philox_accuracy.txt): worst 3.5 units in the bulk, at most 2.5 in any extreme regime; the two
bounded routes differ by at most 0.07 of their bounds; the file runs in 5 s."""
import numpy as np
import pytest
import torch

import philox_truth as T
from step_fixtures import (EXACT_ETA, IPB_PREP_M, WINO_EDGES, ExactProblem, exact_ipb, option, probe_winograd, step_wg, winograd_option,
                           wino_one_chunk_bytes)
from test_gpu_exact_ipb import built, tags
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)
from test_gpu_rows import row_blocks

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNITS_BAR = 9.0
SQ2ETA = 2.0 ** -10  # sqrt(2 EXACT_ETA), exact
# (seed, step, j_offset): plain; high words in seed and step; the column counter wraps after three columns
COUNTERS = [(1, 0, 0), (2**63 + 11, 2**33 + 3, 123456), (0xC0FFEE, 9, 2**32 - 3)]


@pytest.fixture(scope="module")
def fx():
    return T.load()


def fill(P, rows, cols, seed, step, j_offset, ld=None, guard_rows=0):
    """pls_normal_fill of (rows x cols) into a NaN buffer of (rows + guard_rows) x ld; returns the whole buffer"""
    L = P.pkg._lib
    ld = cols if ld is None else ld
    buf = torch.full((rows + guard_rows, ld), NAN, device="cuda")
    L.check(L.load().pls_normal_fill(buf.data_ptr(), ld, rows, cols, seed, step, j_offset, L.stream_ptr()), "pls_normal_fill")
    return buf


# -------------------------------------------------------------------------------------------------------------------------
# 1. the transform against the truth
def _report(name, u):
    k = int(np.argmax(u))
    print(f"philox accuracy: {name:24s} worst {u.max():6.3f} units of 2^-53 |z| over {u.size} elements (at {k})")
    return float(u.max())


def test_fill_bulk_within_nine_units_of_the_truth(P, fx):
    worst = 0.0
    for t, (seed, step, joff) in enumerate(T.BULK_TRIPLES):
        got = fill(P, T.BULK_ROWS, T.BULK_COLS, seed, step, joff).cpu().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, _report(f"bulk {t}", T.units(got, fx["bulk_hi"][t], fx["bulk_lo"][t])))
    assert worst <= UNITS_BAR, f"bulk: {worst:.2f} units"


def test_fill_extremes_within_nine_units_of_the_truth(P, fx):
    """every pair of the extremes through one 8 x 1 fill with j_offset = its column; the relative bar holds the smallest |z| too"""
    L = P.pkg._lib
    cols = fx["ext_col"][0::2]
    buf = torch.full((len(cols), 8), NAN, device="cuda")
    for k, col in enumerate(cols.tolist()):
        L.check(L.load().pls_normal_fill(buf[k].data_ptr(), 1, 8, 1, T.SEARCH_SEED, T.SEARCH_STEP, col, L.stream_ptr()), "pls_normal_fill")
    got = buf.cpu().numpy()
    assert np.isfinite(got).all()
    z = got[np.repeat(np.arange(len(cols)), 2), fx["ext_row"]]
    u = T.units(z, fx["ext_hi"], fx["ext_lo"])
    worst = {}
    for r, name in enumerate(T.REGIMES):
        worst[name] = _report(name, u[fx["ext_regime"] == r])
    over = {k: v for k, v in worst.items() if v > UNITS_BAR}
    assert not over, f"over {UNITS_BAR} units: {over}"


@pytest.mark.parametrize("rows", [1, 3, 4, 5, 12, 13, 16])
def test_fill_behind_guards_and_without_upper_rows(P, fx, rows):
    """a padded leading dimension and row counts whose last pairs have no upper row (rows i and i + 4 share a call): the same
    bits as the full block's rows, hence the truth's within the bar, and not one guard element written"""
    seed, step, joff = T.BULK_TRIPLES[1]
    full = fill(P, T.BULK_ROWS, T.BULK_COLS, seed, step, joff)
    wide = fill(P, rows, T.BULK_COLS, seed, step, joff, ld=T.BULK_COLS + 24, guard_rows=5)
    assert torch.equal(wide[:rows, :T.BULK_COLS], full[:rows]), "the rows of a shorter fill differ from the full block's"
    assert wide[:rows, T.BULK_COLS:].isnan().all() and wide[rows:].isnan().all(), "pls_normal_fill wrote outside rows x cols"
    u = T.units(wide[:rows, :T.BULK_COLS].cpu().numpy(), fx["bulk_hi"][1][:rows], fx["bulk_lo"][1][:rows])
    assert u.max() <= UNITS_BAR


# -------------------------------------------------------------------------------------------------------------------------
# 2. every route draws exactly that stream
def assert_same(drawn, injected, what, bound=None):
    assert torch.isfinite(drawn).all() and torch.isfinite(injected).all(), what
    if bound is None:
        bad = drawn != injected
        if bad.any():
            first = bad.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ between drawn and injected noise, first "
                                 f"(row, column) {first}, rows {torch.unique(bad.nonzero()[:, 0])[:12].tolist()}, "
                                 f"max |diff| {(drawn - injected).abs().max().item():.3e}")
    else:
        diff = (drawn - injected).abs()
        over = diff > bound
        if over.any():
            first = over.nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int(over.sum())} elements over the bound, first (row, column) {first}: "
                                 f"|diff| {diff[tuple(first)].item():.3e}, bound {bound[tuple(first)].item():.3e}")
        ratio = (diff / bound.clamp_min(1e-300)).max().item()
        print(f"{what}: {int((diff != 0).sum())} of {diff.numel()} elements differ, at most {ratio:.3f} of the bound")


def assert_moved(none, *outs, what=""):
    """a step that ignored its noise would return the step without noise: every deviate is non-zero, and sqrt(2 eta) z ~ 1e-3
    next to an update of order one cannot round away"""
    for o in outs:
        assert ((o != none).double().mean() > 0.999), f"{what}: the noise left {int((o == none).sum())} elements unmoved"


def check_route(P, run, rows, j, what, inject=None, bound=None, counters=COUNTERS):
    """run(NoiseSpec) -> the step's output.  ``inject``: Xi -> the route's injected noise (default: Xi itself);
    ``bound``: Xi -> per-element bound (default: bit equality)."""
    NoiseSpec = P.basis.NoiseSpec
    none = run(NoiseSpec(none=True)).clone()
    done = 0
    for seed, step, joff in counters:
        if joff >= 2**31 and j <= 3:
            continue  # (the wrap needs more than three columns)
        xi = fill(P, rows, j, seed, step, joff)
        drawn = run(NoiseSpec(seed=seed, step=step, j_offset=joff)).clone()
        injected = run(NoiseSpec(injected=xi if inject is None else inject(xi))).clone()
        tag = f"{what}, counters ({seed:#x}, {step:#x}, {joff})"
        assert_same(drawn, injected, tag, None if bound is None else bound(xi, injected))
        assert_moved(none, drawn, injected, what=tag)
        done += 1
    assert done >= 2


_onb = {}


def onb(P, mk, n, j):
    """the exact problem of a shape with its basis, cost and device particles, once per module"""
    key = (mk, n, j)
    if key not in _onb:
        if len(_onb) >= 3:
            _onb.clear()
        ex = ExactProblem(mk, n, j, seed=mk + n + j)
        _onb[key] = (ex, ex.basis(P), ex.cost(P), ex.u.cuda())
    return _onb[key]


def route_tags(P, run):
    """the timeline tags of one drawn step (after a first call, which may still build the basis' constants)"""
    spec = P.basis.NoiseSpec(seed=1)
    run(spec)
    return tags(P, lambda: run(spec))


def onb_runner(gb, cost, u, **kw):
    return lambda spec: gb.fused_step(cost, u, EXACT_ETA, noise=spec, **kw)


@pytest.mark.parametrize("chunk", [None, 1000])
def test_plain_general_route(P, chunk):
    """langevin_update_kernel behind the streamed drift, in one chunk of rows and in three"""
    mk, n, j = 133, 3000, 333
    ex, gb, cost, u = onb(P, mk, n, j)
    prev = gb.workspace_bytes
    try:
        if chunk:
            gb.workspace_bytes = P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, chunk)
        run = onb_runner(gb, cost, u, force_generic=True)
        with winograd_option(P, 0):
            names = route_tags(P, run)
            assert "langevin_update" in names and "gemm_langevin_gaussian" not in names and "small_rank_step" not in names, names
            check_route(P, run, mk, j, f"plain general, chunk {chunk}")
    finally:
        gb.workspace_bytes = prev


@pytest.mark.parametrize("mode", [1, 0])
def test_row_block_route(P, mode):
    mk, n, j = 133, 12000, 1100
    ex, gb, cost, u = onb(P, mk, n, j)
    run = onb_runner(gb, cost, u, force_generic=True)
    with row_blocks(P, mode):
        assert "langevin_update" in route_tags(P, run)
        check_route(P, run, mk, j, f"row blocks {mode}")


def test_winograd_route(P):
    """langevin_update_wino_kernel at the route's minimum sizes (all paired rows in one chunk, as tests/test_gpu_winograd.py
    runs its envelope): four (row half, column half) quadrants per thread"""
    mk, n, j = WINO_EDGES[3]
    assert (mk, n, j) == (512, 16384, 2048)
    ex, gb, cost, u = onb(P, mk, n, j)
    ws = wino_one_chunk_bytes(mk, n, j)
    assert probe_winograd(P, gb, cost, u, ws_bytes=ws), "the shape does not take the Winograd route"
    planes = gb._winograd_planes(gb._desc())
    run = lambda spec: step_wg(P, gb, cost, u, EXACT_ETA, planes, noise=spec, ws_bytes=ws)  # noqa: E731
    assert "langevin_update" in route_tags(P, run)
    check_route(P, run, mk, j, "winograd")


@pytest.mark.parametrize("mode,j", [(m, j) for m in (0, 1, 2, 3) for j in (333, 1100)] + [(0, 16400)])
def test_gaussian_fast_path_tilings(P, mode, j):
    """EpiLangevinGaussian: PLS_OPT_KSPLIT_MODE 0 -- 64 x 64 tiles below 256 tiles of 128 x 128, from J = 16400 on (2 x 129) the
    128 x 128 tiles with the direct epilogue inside and the LDS epilogue at the edges; 1 (auto) and 2 -- two k-groups, the draws in
    front of the k-loop; 3 -- one k-group"""
    mk, n = 133, 300
    ex, gb, cost, u = onb(P, mk, n, j)
    run = onb_runner(gb, cost, u, force_generic=False)
    with ksplit(P, mode):
        names = route_tags(P, run)
        assert names == ["gemm_langevin_gaussian"], names
        check_route(P, run, mk, j, f"fast path, k-split mode {mode}, J {j}")


@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("n,mk,j", [(333, 17, 37), (40, 12, 5), (900, 128, 48)])
def test_small_rank_routes(P, mode, n, mk, j):
    """PLS_OPT_SMALL_RANK_STEP 2: the one-launch step; 0: the slab kernels and langevin_update_kernel"""
    ex, gb, cost, u = onb(P, mk, n, j)
    run = onb_runner(gb, cost, u, force_generic=True)
    with option(P, P.pkg._lib.OPT_SMALL_RANK_STEP, mode):
        names = route_tags(P, run)
        if mode == 2:
            assert names == ["small_rank_step"], names
        else:
            assert "small_rank_step" not in names and "langevin_update" in names, names
        check_route(P, run, mk, j, f"small rank {mode}, {n} x {mk} x {j}")


# ---- the inducing-point basis ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", IPB_PREP_M)
def test_ipb_prep_colours_the_streams_draws(P, m):
    """ipb_prep_kernel: E = Lc Xi from its own draws against pls_tri_multiply on the fill, through the one-launch step on U = 0,
    y = 0 (out = 2^-10 E exactly), within the product's forward-error bound (the module's docstring); M = 1: bit-equal"""
    L = P.pkg._lib
    for j in (1, 17, 50):
        ex = exact_ipb(m, 200 + m, j, umax=0, ymax=0)
        gb, cost, u = built(P, ex), ex.cost(P), ex.u.cuda()
        lc = ex.lc.cuda()
        run = lambda spec: gb.fused_step(cost, u, EXACT_ETA, noise=spec, force_generic=True)  # noqa: E731
        with option(P, L.OPT_SMALL_RANK_STEP, 2), option(P, L.OPT_IPB_PREP, 1):
            assert route_tags(P, run) == ["ipb_prep", "small_rank_step"]
            check_route(P, run, m, j, f"ipb_prep, M {m}, J {j}", inject=gb._chol.colour,
                        bound=lambda xi, out: (m + 2) * 2.0 ** -53 * (lc.abs() @ xi.abs()) * SQ2ETA)
            if m == 1:
                check_route(P, run, m, j, f"ipb_prep, M 1, J {j}", inject=gb._chol.colour)


@pytest.mark.parametrize("m,n,j", [(64, 300, 40), (200, 1500, 333)])
def test_ipb_two_launch_gaussian_step(P, m, n, j):
    """pls_ipb_step, Gaussian / identity: dS with white draws in EpiLangevinGaussian, then Lc dS -- against the coloured noise added
    behind the product, within the bound of the module's docstring"""
    ex = exact_ipb(m, n, j)
    gb, cost, u = built(P, ex), ex.cost(P), ex.u.cuda()
    lc = ex.lc.cuda()
    run = lambda spec: gb.fused_step(cost, u, EXACT_ETA, noise=spec)  # noqa: E731
    names = route_tags(P, run)
    assert "gemm_langevin_gaussian" in names and "langevin_update" not in names, names
    ds = gb.whitened_step(cost, gb.whiten(u), EXACT_ETA, noise=P.basis.NoiseSpec(none=True)).abs()
    check_route(P, run, m, j, f"two-launch Gaussian step {m} x {n} x {j}", inject=gb._chol.colour,
                bound=lambda xi, out: (m + 3) * 2.0 ** -53 * (lc.abs() @ (ds + SQ2ETA * xi.abs())) + 2.0 ** -53 * out.abs())


@pytest.mark.parametrize("m,n,j", [(64, 300, 40), (200, 1500, 333)])
def test_ipb_whitened_step(P, m, n, j):
    """pls_ipb_whitened_step, Gaussian / identity: white noise either way"""
    ex = exact_ipb(m, n, j)
    gb, cost, s = built(P, ex), ex.cost(P), ex.s.cuda()
    run = lambda spec: gb.whitened_step(cost, s, EXACT_ETA, noise=spec)  # noqa: E731
    assert route_tags(P, run) == ["gemm_langevin_gaussian"]
    check_route(P, run, m, j, f"whitened step {m} x {n} x {j}")


@pytest.mark.parametrize("n,m,j", [(50, 1, 8), (100, 4, 64), (333, 16, 37)])
def test_ipb_whitened_generic_step(P, n, m, j):
    """pls_ipb_whitened_generic_step: the prior-row instantiations of the one-launch step; M = 1 and 4: lone lower rows only"""
    ex = exact_ipb(m, n, j)
    gb, cost, s = built(P, ex), ex.cost(P), ex.s.cuda()
    assert gb.whitened_generic_applies(cost, j, force_generic=True)
    run = lambda spec: gb.whitened_step(cost, s, EXACT_ETA, noise=spec, force_generic=True)  # noqa: E731
    assert route_tags(P, run) == ["small_rank_step"]
    check_route(P, run, m, j, f"whitened generic step {n} x {m} x {j}")
    gb.zero_step_sync()


def test_ipb_general_route(P):
    """M = 200, J = 65: the fill and the triangular product the route launches for its own draws are pls_normal_fill and
    pls_tri_multiply on the same operands (an odd leading dimension: neither takes the balanced kernel)"""
    m, n, j = 200, 300, 65
    ex = exact_ipb(m, n, j)
    gb, cost, u = built(P, ex, explicit_inverse=True), ex.cost(P), ex.u.cuda()
    run = lambda spec: gb.fused_step(cost, u, EXACT_ETA, noise=spec, force_generic=True)  # noqa: E731
    names = route_tags(P, run)
    # (the route's fill and update launches carry no tag of their own: the streamed drift's do)
    assert "gemm_cost_deriv" in names and not {"gemm_langevin_gaussian", "small_rank_step", "ipb_prep"} & set(names), names
    check_route(P, run, m, j, "inducing-point general route", inject=gb._chol.colour)


# ---- run-time step base, column blocks, output forms: one route of each basis ------------------------------------------------
def _entries(P):
    """(name, rows, J, entry(noise=..., **kw) -> output, particles) of the fast path of the orthonormal basis (k-split, the
    default at this size) and of the whitened step of the inducing-point basis"""
    mk, n, j = 133, 300, 334
    ex, gb, cost, u = onb(P, mk, n, j)
    yield "fast path", mk, j, (lambda **kw: gb.fused_step(cost, kw.pop("u", u), kw.pop("eta", EXACT_ETA), **kw)), u
    ei = exact_ipb(64, 300, 40)
    gi, ci, s = built(P, ei), ei.cost(P), ei.s.cuda()
    yield "whitened step", 64, 40, (lambda **kw: gi.whitened_step(ci, kw.pop("u", s), kw.pop("eta", EXACT_ETA), **kw)), s


def test_step_base_is_added_at_run_time(P):
    """a device int64 added to ``step`` inside the kernel (a captured graph's counter) draws the block of step + base: a base that
    carries into the high word, and one added to a step with a high word of its own"""
    NoiseSpec = P.basis.NoiseSpec
    for name, rows, j, entry, _ in _entries(P):
        for seed, step, joff, base in [(7, 3, 5, 2**33 - 2), (2**63 + 11, 2**33 + 3, 123456, 2**31)]:
            word = torch.tensor([base], dtype=torch.int64, device="cuda")
            drawn = entry(noise=NoiseSpec(seed=seed, step=step, j_offset=joff, step_base=word))
            xi = fill(P, rows, j, seed, step + base, joff)
            assert_same(drawn, entry(noise=NoiseSpec(injected=xi)), f"{name}: step {step:#x} + base {base:#x}")
            assert not torch.equal(drawn, entry(noise=NoiseSpec(seed=seed, step=step, j_offset=joff))), f"{name}: the base was ignored"


def test_blocks_draw_the_column_inside_the_block(P):
    """BlockSpec: the Philox column is j_offset + the column inside the block, so the injected Xi is the block's fill tiled
    across the blocks, and blocks with equal step sizes and equal particles return equal outputs"""
    NoiseSpec = P.basis.NoiseSpec
    for name, rows, j, entry, u in _entries(P):
        bc = j // 2
        ub = u[:, :bc].repeat(1, 2).contiguous()
        blocks = P.basis.BlockSpec(bc, torch.full((2,), EXACT_ETA, device="cuda"))
        for seed, step, joff in COUNTERS:
            xi = fill(P, rows, bc, seed, step, joff).repeat(1, 2).contiguous()
            drawn = entry(u=ub, eta=0.0, blocks=blocks, noise=NoiseSpec(seed=seed, step=step, j_offset=joff))
            assert_same(drawn, entry(u=ub, eta=0.0, blocks=blocks, noise=NoiseSpec(injected=xi)), f"{name}: blocks of {bc} columns")
            assert torch.equal(drawn[:, :bc], drawn[:, bc:]), f"{name}: two equal blocks returned different outputs"
            plain = entry(u=ub, noise=NoiseSpec(seed=seed, step=step, j_offset=joff))
            assert torch.equal(plain[:, :bc], drawn[:, :bc]) and not torch.equal(plain[:, bc:], drawn[:, bc:]), \
                f"{name}: without blocks the second half draws columns {bc} .."


def test_output_forms_draw_the_same_noise(P):
    """run_forms' three forms: out of place, into a strided buffer behind NaN guards, as the new state"""
    NoiseSpec = P.basis.NoiseSpec
    for name, rows, j, entry, u in _entries(P):
        for seed, step, joff in COUNTERS:
            specs = (NoiseSpec(seed=seed, step=step, j_offset=joff), NoiseSpec(injected=fill(P, rows, j, seed, step, joff)))
            delta = [entry(noise=s) for s in specs]
            assert_same(*delta, f"{name}: out of place")
            wide = [torch.full((rows, j + 64), NAN, device="cuda") for _ in specs]
            for w, s in zip(wide, specs):
                entry(noise=s, out=w[:, :j])
                assert w[:, j:].isnan().all(), f"{name}: the step wrote past J"
            assert_same(wide[0][:, :j], wide[1][:, :j], f"{name}: strided output")
            assert torch.equal(wide[0][:, :j], delta[0]), f"{name}: the strided output differs from the fresh one"
            new = [entry(noise=s, new_state=True) for s in specs]
            assert_same(*new, f"{name}: new state")
            assert not torch.equal(new[0], delta[0])
