"""GPU: every kernel and every step route of the inducing-point basis on exact problems (step_fixtures.ExactIpbProblem):
k(Z,Z) = Lc Lc^T with a constructed factor whose pivots are powers of four and whose inverse is known in closed form, small
integer k(Z,X), particles, noise and targets, variance 1/4 and a power-of-two step size.  Nothing rounds on these inputs, in
any summation order (the fixture proves it from the data), so the conditioning of k(Z,Z) does not enter and every result must
equal plain fp64 torch on the host bit for bit (torch.equal): the factorisation at its block edges, the inverse factor, the
substitution kernel, the triangular products (plain, balanced on one scratch twice, k-split), the explicit inverse, the
one-launch solve, the four step routes of pls_ipb_step and the whitened entries, three consecutive whitened steps included.
Each route is shown to have run by poisoning with NaN the operand only it reads (NaN out) and the operands it must not read
(bit-equal output), and by the kernel tags of its launches where operands cannot tell two routes apart.

Energies: bit-equal where the fixture shows the quadratic forms fit one mantissa (energy_exact), else per particle at 1e-13."""
import copy

import pytest
import torch

from step_fixtures import (BLOCK_ETAS, EXACT_ETA, IPB_CHAIN_CASES, IPB_FACTOR_M, IPB_ONE_LAUNCH_SHAPES, IPB_PREP_M, IPB_SOLVE_CASES,
                           IPB_STEP_SHAPES, IPB_GENERAL_CASES, IPB_WHITENED_GENERIC_SHAPES, assert_exact, exact_ipb, option, run_forms,
                           spread_columns)
from test_gpu_ksplit import ksplit
from test_gpu_parity import P, _f64_default  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NAN = float("nan")
_factors = {}


def sample(j):
    if j <= 512:
        return None
    return torch.unique(torch.cat([spread_columns(j), torch.tensor([j - 1])]))


def factor(P, ex, host=False):
    """the device factorisation of the problem's k(Z,Z) (or its constructed factor uploaded), once per M, with the inverse factor"""
    from projected_langevin_sampling_amd import _chol

    key = (ex.m, ex.seed, host)
    if key not in _factors:
        f = _chol.factor_from_host(ex.lc) if host else _chol.cholesky_factor(ex.kzz.cuda())
        _factors[key] = f.build_inverse()
    return _factors[key]


def nan_like(t):
    base = t if t._base is None else t._base
    return torch.full_like(base, NAN).as_strided(t.shape, t.stride(), t.storage_offset())


def poisoned(gb, *names):
    """A copy of the basis whose descriptor carries NaN in the named operands: Pt, Q, B, W, Awa, Linv (with LinvT), S (Sf, Sb)."""
    g = copy.copy(gb)
    g.__dict__.pop("_desc_cache", None)
    g._chol = copy.copy(gb._chol)
    for name in names:
        if name == "Linv":
            g._chol.Linv, g._chol.LinvT = nan_like(gb._chol.Linv), nan_like(gb._chol.LinvT)
        elif name == "S":
            g._chol.Sf, g._chol.Sb = nan_like(gb._chol.Sf), nan_like(gb._chol.Sb)
        else:
            assert getattr(gb, "_" + name) is not None, f"the basis has no {name}"
            setattr(g, "_" + name, nan_like(getattr(gb, "_" + name)))
    return g


def probe(gb, reads, skips, run, check, what):
    """``run(basis)`` -> output: NaN with any operand of ``reads`` poisoned, ``check(output)`` (bit-equal) with all of ``skips``"""
    for name in reads:
        assert run(poisoned(gb, name)).isnan().any(), f"{what}: the route did not read {name}"
    check(run(poisoned(gb, *skips)), f"{what}: with {', '.join(skips)} poisoned")


def tags(P, fn):
    with P.pkg._lib.Timeline(256) as tl:
        fn()
    return sorted(tl.summary())


# -------------------------------------------------------------------------------------------------------------------------
# building blocks
@pytest.mark.parametrize("m", IPB_FACTOR_M)
def test_factor_and_inverse_factor(P, m):
    """pls_chol_factor at the block edges of chol.hip (panel 64, substitution block 128, strip depth 32; each edge -1, 0, +1),
    pls_chol_build_inverse through the device's own substitution operators and through pls_chol_build_operators' (uploaded
    factor)"""
    ex = exact_ipb(m, 16, 8)
    for host in (False, True):
        f = factor(P, ex, host)
        assert f.jitter == 0.0
        assert torch.equal(f.Lc.cpu(), ex.lc), f"Lc (uploaded {host})"  # (exact zeros above the diagonal included)
        assert torch.equal(f.LcT.cpu(), ex.lc.T), "LcT"
        assert torch.equal(f.Linv.cpu(), ex.linv), f"Linv (uploaded {host})"
        assert torch.equal(f.LinvT.cpu(), ex.linv.T), f"LinvT (uploaded {host})"


def _solve(P, f, u_host, scratch=True, forward=False):
    """pls_chol_solve_ws / pls_chol_forward_solve on a strided right-hand side into a strided output, both inside NaN guard
    columns: the guards of the output must come back untouched (and those of the input never reach the result)."""
    L, lib = P.pkg._lib, P.pkg._lib.load()
    m, j = u_host.shape
    wide_u = torch.full((m, j + 16), NAN, device="cuda")
    wide_v = torch.full((m, j + 32), NAN, device="cuda")
    u, v = wide_u[:, 8:8 + j], wide_v[:, 16:16 + j]
    u.copy_(u_host)
    d = f.desc()
    if not scratch:
        d.tri_scratch, d.tri_scratch_bytes = None, 0
    if forward:
        L.check(lib.pls_chol_forward_solve(d, u.data_ptr(), L.ld(u), j, v.data_ptr(), L.ld(v), L.stream_ptr()), "forward_solve")
    else:
        ws = torch.empty(m * j, device="cuda")
        L.check(lib.pls_chol_solve_ws(d, u.data_ptr(), L.ld(u), j, v.data_ptr(), L.ld(v), ws.data_ptr(), ws.numel() * 8,
                                      L.stream_ptr()), "solve_ws")
    assert wide_v[:, :16].isnan().all() and wide_v[:, 16 + j:].isnan().all(), "a solve wrote outside its J columns"
    return v.cpu()


def _flags_zero(f):
    sc = f.tri_scratch()
    return sc is None or bool((sc[: f.TRI_FLAG_BYTES // 8] == 0).all())


@pytest.mark.parametrize("m,j", IPB_SOLVE_CASES)
def test_solves_and_products(P, m, j):
    """V = k(Z,Z)^-1 U, S = Lc^-1 U and Lc xi through every solve route: substitution (PLS_OPT_SOLVE_MODE 0; device and uploaded
    operators), inverse-factor products (1) with and without a scratch, balanced or not, k-split modes 1 / 2 / 3 -- twice on
    one scratch, whose flag words must come back zero."""
    L = P.pkg._lib
    ex = exact_ipb(m, 16, j)
    s_want, v_want = ex.s, ex.solve(ex.u)

    def check(f, what, **kw):
        assert torch.equal(_solve(P, f, ex.u, **kw), v_want), f"{what}: solve"
        assert torch.equal(_solve(P, f, ex.u, forward=True, **kw), s_want), f"{what}: forward solve"
        assert _flags_zero(f), f"{what}: the flag words of the scratch were left set"

    f = factor(P, ex)
    with option(P, L.OPT_SOLVE_MODE, 0):
        assert "tri_solve" in tags(P, lambda: f.solve(ex.u.cuda()))
        check(f, "substitution")
        check(factor(P, ex, host=True), "substitution, uploaded factor")
    with option(P, L.OPT_SOLVE_MODE, 1):
        assert "tri_solve" not in tags(P, lambda: f.solve(ex.u.cuda()))
        for bal in (1, 0):
            with option(P, L.OPT_TRI_BALANCE, bal):
                check(f, f"products, balance {bal}")
                check(f, f"products, balance {bal}, again on the same scratch")
        check(f, "products without a scratch", scratch=False)
        for mode in (1, 2, 3):
            with ksplit(P, mode):
                check(f, f"products, k-split {mode}")
        check(factor(P, ex, host=True), "products, uploaded factor")
    assert torch.equal(f.colour(ex.xi.cuda()).cpu(), ex.e), "Lc xi (pls_tri_multiply)"
    assert torch.equal(f.solve(ex.u.cuda()).cpu(), v_want) and torch.equal(f.forward_solve(ex.u.cuda()).cpu(), s_want)


def test_product_solves_read_the_inverse_factor_and_substitution_its_operators(P):
    L = P.pkg._lib
    ex = exact_ipb(200, 16, 65)
    f = factor(P, ex)
    for mode, reads, skips in ((1, "Linv", "S"), (0, "S", "Linv")):
        bad, ok = copy.copy(f), copy.copy(f)
        for g, name in ((bad, reads), (ok, skips)):
            if name == "Linv":
                g.Linv, g.LinvT = nan_like(f.Linv), nan_like(f.LinvT)
            else:
                g.Sf, g.Sb = nan_like(f.Sf), nan_like(f.Sb)
        with option(P, L.OPT_SOLVE_MODE, mode):
            assert _solve(P, bad, ex.u).isnan().any() and _solve(P, bad, ex.u, forward=True).isnan().any(), (mode, reads)
            assert torch.equal(_solve(P, ok, ex.u), ex.solve(ex.u)) and torch.equal(_solve(P, ok, ex.u, forward=True), ex.s)


# -------------------------------------------------------------------------------------------------------------------------
# the routes of pls_ipb_step
_bases = {}


def built(P, ex, **kw):
    key = (ex.m, ex.n, ex.j, ex.seed, tuple(sorted(kw.items())))
    if key not in _bases:
        if len(_bases) >= 4:
            _bases.clear()
        _bases[key] = ex.basis(P, **kw)
        assert torch.equal(_bases[key]._chol.Lc.cpu(), ex.lc) and torch.equal(_bases[key]._chol.Linv.cpu(), ex.linv)
    return _bases[key]


def _stepper(P, ex, cost, cols, **kw):
    u, e = ex.u.cuda(), P.basis.NoiseSpec(injected=ex.injected.cuda())

    def run(gb):
        return gb.fused_step(cost, u, EXACT_ETA, noise=e, **kw)

    def check(got, what):
        assert_exact(ex, got, cols, what=what)

    return run, check


@pytest.mark.parametrize("m,n,j", IPB_STEP_SHAPES)
@pytest.mark.parametrize("host_factor", [False, True])
def test_whitened_routes(P, m, n, j, host_factor):
    """Gaussian / identity, the default: dS from U through Pt = Lc^-T Q (no energies), or forward solve + Q S (energies asked
    for, or PLS_OPT_IPB_STEP_OPERATOR 0; its solve by products or by substitution), then Lc dS"""
    L = P.pkg._lib
    ex = exact_ipb(m, n, j)
    gb, cost, cols = built(P, ex, host_factor=host_factor), ex.cost(P), sample(j)
    gb._prepare_for(cost)
    assert torch.equal(gb._Q.cpu(), ex.q) and torch.equal(gb._Pt.cpu(), ex.linv.T @ ex.q), "the whitened operators"
    assert torch.equal(gb._B.cpu(), ex.kzx @ ex.kzx.T), "B = k(Z,X) k(X,Z)"
    run_forms(P, ex, gb, cost, cols, "whitened", force_generic=False)
    probe(gb, ["Pt"], ["Q", "B", "Linv", "S"], *_stepper(P, ex, cost, cols), "whitened / Pt")
    e = torch.empty(j, device="cuda")
    probe(gb, ["Q", "Linv"], ["Pt", "B", "S"], *_stepper(P, ex, cost, cols, input_energy=e), "whitened / Q for the energies")
    with option(P, L.OPT_IPB_STEP_OPERATOR, 0):
        run_forms(P, ex, gb, cost, cols, "whitened / Q", force_generic=False)
        probe(gb, ["Q", "Linv"], ["Pt", "B", "S"], *_stepper(P, ex, cost, cols), "whitened / Q")
        with option(P, L.OPT_SOLVE_MODE, 0):
            run_forms(P, ex, gb, cost, cols, "whitened / Q, substitution", force_generic=False)
            probe(gb, ["Q", "S"], ["Pt", "B", "Linv"], *_stepper(P, ex, cost, cols), "whitened / Q, substitution")


@pytest.mark.parametrize("m,n,j", IPB_STEP_SHAPES)
def test_fast_route(P, m, n, j):
    """a descriptor without Q: V = k(Z,Z)^-1 U, B V / sigma2, the update; and the same with the explicit inverse W"""
    L = P.pkg._lib
    ex = exact_ipb(m, n, j)
    cost, cols = ex.cost(P), sample(j)
    gb = copy.copy(built(P, ex, explicit_inverse=True))
    gb.whitened = False
    gb._prepare_for(cost)
    assert torch.equal(gb._W.cpu(), ex.linv.T @ ex.linv), "W = k(Z,Z)^-1 (host cholesky_inverse of the device's factor)"
    run_forms(P, ex, gb, cost, cols, "fast", force_generic=False)
    probe(gb, ["B", "Linv"], ["S", "W"], *_stepper(P, ex, cost, cols), "fast")
    with option(P, L.OPT_SOLVE_MODE, 0):
        run_forms(P, ex, gb, cost, cols, "fast, substitution", force_generic=False)
        probe(gb, ["B", "S"], ["Linv", "W"], *_stepper(P, ex, cost, cols), "fast, substitution")
    with option(P, L.OPT_IPB_EXPLICIT_INVERSE, 1):
        run_forms(P, ex, gb, cost, cols, "fast, explicit inverse", force_generic=False)
        probe(gb, ["B", "W"], ["Linv", "S"], *_stepper(P, ex, cost, cols), "fast, explicit inverse")
        whitened = built(P, ex, explicit_inverse=True)  # (the whitened route steps aside for the A/B option)
        whitened._prepare_for(cost)
        probe(whitened, ["B", "W"], ["Linv", "S", "Q", "Pt"], *_stepper(P, ex, cost, cols), "explicit inverse on a whitened basis")


@pytest.mark.parametrize("m,n,j,chunk", IPB_GENERAL_CASES)
def test_general_route(P, m, n, j, chunk):
    """force_generic: solve, the drift streamed over row chunks (one; three in a workspace sized for N / 3 rows) and split-K
    slabs (N = 300: one; N = 20000: several), update"""
    L = P.pkg._lib
    ex = exact_ipb(m, n, j)
    gb, cost, cols = built(P, ex, explicit_inverse=True), ex.cost(P), sample(j)
    if chunk:
        gb = copy.copy(gb)
        gb.workspace_bytes = L.load().pls_ipb_step_workspace_bytes(gb._desc(), j, chunk)
    gb._prepare_for(cost)
    run_forms(P, ex, gb, cost, cols, f"general, chunk {chunk}")
    probe(gb, ["Linv"], ["S", "W", "B", "Q", "Pt"], *_stepper(P, ex, cost, cols, force_generic=True), "general")
    f = gb.calculate_untransformed_train_prediction_samples(ex.u.cuda())
    assert torch.equal(f.cpu(), ex.kzx.T @ ex.solve(ex.u)), "pls_ipb_forward"
    e = gb.fused_particle_energy(cost, ex.u.cuda(), force_generic=True)
    assert_exact(ex, gb.fused_step(cost, ex.u.cuda(), EXACT_ETA, noise=P.basis.NoiseSpec(injected=ex.injected.cuda()), force_generic=True),
                 cols, energy=e, what="pls_ipb_energy")
    if chunk:
        return
    with option(P, L.OPT_SOLVE_MODE, 0):
        run_forms(P, ex, gb, cost, cols, "general, substitution")
        probe(gb, ["S"], ["Linv", "W"], *_stepper(P, ex, cost, cols, force_generic=True), "general, substitution")
    with option(P, L.OPT_IPB_EXPLICIT_INVERSE, 1):
        run_forms(P, ex, gb, cost, cols, "general, explicit inverse")
        probe(gb, ["W"], ["Linv", "S"], *_stepper(P, ex, cost, cols, force_generic=True), "general, explicit inverse")


@pytest.mark.parametrize("n,m,j", IPB_ONE_LAUNCH_SHAPES)
def test_one_launch_route(P, n, m, j):
    """at most 128 inducing points, launch-bound: the one-launch step behind the one-launch solve (csrc/ipb_prep.h), or behind
    the two triangular products (PLS_OPT_IPB_PREP 0)"""
    L = P.pkg._lib
    ex = exact_ipb(m, n, j)
    gb, cost = built(P, ex), ex.cost(P)
    run, check = _stepper(P, ex, cost, None, force_generic=True)
    with option(P, L.OPT_SMALL_RANK_STEP, 2):
        assert tags(P, lambda: run(gb)) == ["ipb_prep", "small_rank_step"]  # two launches, nothing else
        run_forms(P, ex, gb, cost, None, "one launch, ipb_prep")
        probe(gb, ["Linv"], ["S"], run, check, "one launch, ipb_prep")
        with option(P, L.OPT_IPB_PREP, 0):
            names = tags(P, lambda: run(gb))
            assert "small_rank_step" in names and "ipb_prep" not in names and "tri_solve" not in names, names
            run_forms(P, ex, gb, cost, None, "one launch, two products")
            probe(gb, ["Linv"], ["S"], run, check, "one launch, two products")
            with option(P, L.OPT_SOLVE_MODE, 0):
                names = tags(P, lambda: run(gb))
                assert "small_rank_step" in names and "tri_solve" in names and "ipb_prep" not in names, names
                run_forms(P, ex, gb, cost, None, "one launch, substitution")
                probe(gb, ["S"], ["Linv"], run, check, "one launch, substitution")


@pytest.mark.parametrize("m", IPB_PREP_M)
def test_one_launch_solve_at_every_rank(P, m):
    """csrc/ipb_prep.h for ranks on both sides of every 16-row tile edge and ragged column counts, injected noise: the step
    behind it is exact only if its V is (the launch's own Philox colouring stays with
    test_solve_and_coloured_noise_in_one_launch_at_every_rank)"""
    L = P.pkg._lib
    for j in (1, 17, 50):
        ex = exact_ipb(m, 200 + m, j)
        gb, cost = built(P, ex), ex.cost(P)
        run, check = _stepper(P, ex, cost, None, force_generic=True)
        with option(P, L.OPT_SMALL_RANK_STEP, 2):
            for prep in (1, 0):
                with option(P, L.OPT_IPB_PREP, prep):
                    assert ("ipb_prep" in tags(P, lambda: run(gb))) == bool(prep)
                    e = torch.empty(j, device="cuda")
                    got = gb.fused_step(cost, ex.u.cuda(), EXACT_ETA, noise=P.basis.NoiseSpec(injected=ex.injected.cuda()),
                                        force_generic=True, input_energy=e)
                    assert_exact(ex, got, energy=e, what=f"m {m}, j {j}, ipb_prep {prep}")


# -------------------------------------------------------------------------------------------------------------------------
# whitened coordinates
def assert_whitened(ex, got, cols=None, energy=None, what="", **kw):
    want, e_want = ex.whitened_step(cols, **kw)
    got = got.cpu() if cols is None else got.cpu()[:, cols]
    assert torch.isfinite(got).all(), what
    bad = (got != want).any(dim=1).nonzero().flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} rows differ from the exact whitened step, first {bad[:8].tolist()}, " \
                             f"max |diff| {(got - want).abs().max().item():.3e}"
    if energy is not None:
        e = energy.cpu() if cols is None else energy.cpu()[cols]
        rel = ((e - e_want).abs() / e_want.abs()).max().item()
        assert rel <= 1e-13, f"{what}: energy by-product, relative error {rel:.2e}"
        if ex.energy_exact:
            assert torch.equal(e, e_want), f"{what}: energy by-product differs from the exact one, relative error {rel:.2e}"


def run_whitened_forms(P, ex, gb, cost, cols, what, **kw):
    """run_forms for the entries that step whitened particles (white injected noise)"""
    j, s, xi = ex.j, ex.s.cuda(), P.basis.NoiseSpec(injected=ex.xi.cuda())
    e = torch.full((j,), NAN, device="cuda")
    got = gb.whitened_step(cost, s, EXACT_ETA, noise=xi, input_energy=e, **kw)
    assert_whitened(ex, got, cols, energy=e, what=f"{what}: out of place")
    wide = torch.full((ex.m, j + 64), NAN, device="cuda")
    out = wide[:, :j]
    gb.whitened_step(cost, s, EXACT_ETA, noise=xi, out=out, **kw)
    assert_whitened(ex, out, cols, what=f"{what}: strided output")
    assert wide[:, j:].isnan().all(), f"{what}: the step wrote past J"
    new = gb.whitened_step(cost, s, EXACT_ETA, noise=xi, new_state=True, **kw)
    assert_whitened(ex, new, cols, new_state=True, what=f"{what}: new state")
    bc = -(-j // len(BLOCK_ETAS))
    blocks = P.basis.BlockSpec(bc, torch.tensor(BLOCK_ETAS, device="cuda"))
    got = gb.whitened_step(cost, s, 0.0, noise=xi, blocks=blocks, new_state=True, **kw)
    etas = torch.tensor(BLOCK_ETAS)[torch.arange(j) // bc]
    assert_whitened(ex, got, cols, eta=etas if cols is None else etas[cols], new_state=True, what=f"{what}: blocks")
    assert torch.equal(got[:, bc:2 * bc].cpu(), ex.s[:, bc:2 * bc]), f"{what}: a frozen block moved"
    with pytest.raises(AssertionError, match="alias"):
        gb.whitened_step(cost, s, EXACT_ETA, noise=xi, out=s, **kw)
    r = gb._route(cost, j, kw.get("force_generic", False), whitened=True)
    bd = None
    if r.one_launch:
        bd = blocks.desc()
        bd.step_sync = gb._step_sync(j, s.device).data_ptr()
    with pytest.raises(P.pkg._lib.PlsHipError):  # in place: the entries refuse an output that aliases the particles
        ws = torch.empty(r.ws_bytes // 8 + 1, device="cuda")
        P.pkg._lib.check(r.call(bd, s.data_ptr(), j, j, EXACT_ETA, xi.desc(), s.data_ptr(), j, 0, None, ws.data_ptr(), r.ws_bytes,
                                P.pkg._lib.stream_ptr()), "in place")
    gb.zero_step_sync()


@pytest.mark.parametrize("m,n,j", IPB_STEP_SHAPES)
def test_whiten_unwhiten_and_the_whitened_step(P, m, n, j):
    ex = exact_ipb(m, n, j)
    gb, cost, cols = built(P, ex), ex.cost(P), sample(j)
    u = ex.u.cuda()
    s = gb.whiten(u)
    assert torch.equal(s.cpu(), ex.s), "whiten"
    assert torch.equal(gb.unwhiten(s).cpu(), ex.u), "unwhiten(whiten(U)) is not U"
    gb._prepare_for(cost)

    def same(got, what):
        assert torch.equal(got.cpu(), ex.s), what

    probe(gb, ["Linv"], ["S", "Q", "Pt", "B"], lambda g: g.whiten(u), same, "whiten")
    run_whitened_forms(P, ex, gb, cost, cols, "whitened step")
    xi = P.basis.NoiseSpec(injected=ex.xi.cuda())
    probe(gb, ["Q"], ["Pt", "B", "Linv", "S"], lambda g: g.whitened_step(cost, s, EXACT_ETA, noise=xi),
          lambda got, what: assert_whitened(ex, got, cols, what=what), "whitened step")
    e = gb.whitened_particle_energy(cost, s)
    assert_whitened(ex, gb.whitened_step(cost, s, EXACT_ETA, noise=xi), cols, energy=e, what="pls_ipb_whitened_energy")


@pytest.mark.parametrize("m,n,j,kw", IPB_CHAIN_CASES)
def test_three_consecutive_whitened_steps(P, m, n, j, kw):
    """the training loop's state: three steps of pls_ipb_whitened_step, and of its _blocks entry with one frozen block, each
    with fresh injected noise, against the host chain -- the fixture proves the growing state stays exact"""
    ex = exact_ipb(m, n, j, chain=3, **kw)
    gb, cost = built(P, ex), ex.cost(P)
    bc = -(-j // 4)
    etas = torch.tensor([ex.eta, 0.0, ex.eta, ex.eta])
    blocks = P.basis.BlockSpec(bc, etas.cuda())
    col_etas = etas[torch.arange(j) // bc]
    plain = blocked = gb.whiten(ex.u.cuda())
    want = want_b = ex.s
    for k in range(3):
        xi = ex.chain_noise(k)
        spec = P.basis.NoiseSpec(injected=xi.cuda())
        plain = gb.whitened_step(cost, plain, ex.eta, noise=spec, new_state=True)
        want, _ = ex.whitened_step(eta=ex.eta, new_state=True, state=want, xi=xi)
        assert torch.equal(plain.cpu(), want), f"step {k}: max |diff| {(plain.cpu() - want).abs().max().item():.3e}"
        blocked = gb.whitened_step(cost, blocked, 0.0, noise=spec, new_state=True, blocks=blocks)
        want_b, _ = ex.whitened_step(eta=col_etas, new_state=True, state=want_b, xi=xi)
        assert torch.equal(blocked.cpu(), want_b), f"blocks, step {k}"
    assert torch.equal(blocked[:, bc:2 * bc].cpu(), ex.s[:, bc:2 * bc]), "a frozen block moved"
    assert torch.equal(gb.unwhiten(plain).cpu(), ex.lc @ want), "unwhiten of the final state"


@pytest.mark.parametrize("n,m,j", IPB_WHITENED_GENERIC_SHAPES)
def test_whitened_generic_step(P, n, m, j):
    """pls_ipb_whitened_generic_step: the one-launch step over Awa = k(X,Z) Lc^-T over sqrt(M) Lc^-T (M a power of four: the
    square root is exact)"""
    ex = exact_ipb(m, n, j)
    gb, cost = built(P, ex), ex.cost(P)
    assert gb.whitened_generic_applies(cost, j, force_generic=True)
    assert torch.equal(gb._Awa.cpu(), torch.cat([ex.kzx.T @ ex.linv.T, m ** 0.5 * ex.linv.T])), "Awa"
    s, xi = ex.s.cuda(), P.basis.NoiseSpec(injected=ex.xi.cuda())
    assert tags(P, lambda: gb.whitened_step(cost, s, EXACT_ETA, noise=xi, force_generic=True)) == ["small_rank_step"]
    run_whitened_forms(P, ex, gb, cost, None, "whitened generic", force_generic=True)
    gb._prepare_for(cost)
    probe(gb, ["Awa"], ["Linv", "S", "Q", "Pt", "B"], lambda g: g.whitened_step(cost, s, EXACT_ETA, noise=xi, force_generic=True),
          lambda got, what: assert_whitened(ex, got, what=what), "whitened generic")
