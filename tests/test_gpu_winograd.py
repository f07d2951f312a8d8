"""GPU: the Strassen-Winograd route of the orthonormal basis' general step (csrc/winograd.h, PLS_OPT_WINOGRAD) against the plain
route on the same inputs: every cost/link pair with and without the energy by-product, per-block step sizes, a J-shard's
j_offset, N streamed in several chunks of paired rows, and shapes outside the route, which must not move a bit.  That the
route ran is proven by the NaN-plane probe (step_fixtures.probe_winograd), not by the two routes rounding differently.  The
route's envelope -- edge tiles in M_k, J and N, its minimum sizes, one and three chunks, one and several slabs, blocks across
J/2, a strided particle matrix -- is checked exactly (step_fixtures.ExactProblem), and on a graded RBF spectrum at the
headline shape every eigen-direction of D = A G is held to a per-row bound."""
import pytest
import torch

import bench
from step_fixtures import (EXACT_ETA, WINO_EDGES, WINO_OUTSIDE, WINO_THREE_CHUNKS, ExactProblem, probe_winograd, spread_columns,
                           step_wg, winograd_option, wino_one_chunk_bytes)
from test_gpu_parity import TOL, P, _f64_default, make_costs, relerr, row_relerr  # noqa: F401
from test_winograd_host import _winograd

pytestmark = pytest.mark.gpu


def _problem(P, n, mk, j, seed=0):
    """A basis given by a random projection (exactly mk functions), targets of every cost family, prior-scaled particles."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(mk, n, generator=g, dtype=torch.float64) / mk ** 0.5
    lam = 0.5 + torch.rand(mk, generator=g, dtype=torch.float64)
    gb = P.basis.OrthonormalBasis.from_projection(a.cuda(), lam.cuda(), poison_padding=True)
    gb.workspace_bytes = 4 << 30
    fstar = torch.sin(torch.linspace(-3.0, 3.0, n, dtype=torch.float64))
    y = fstar + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    u = (torch.randn(mk, j, generator=g, dtype=torch.float64) * lam.sqrt()[:, None]).cuda()
    return gb, y, fstar, g, u


def _with_option(P, value, fn):
    lib, L = P.pkg._lib.load(), P.pkg._lib
    assert lib.pls_get_option(L.OPT_WINOGRAD) == 1
    L.check(lib.pls_set_option(L.OPT_WINOGRAD, value), "pls_set_option")
    try:
        return fn()
    finally:
        L.check(lib.pls_set_option(L.OPT_WINOGRAD, 1), "pls_set_option")


def _both_routes(P, fn):
    """(plain route, Winograd route) of the same call."""
    plain = _with_option(P, 0, fn)
    wino = fn()
    return plain, wino


# N = 40000: the plain route's workspace for all rows (what the basis asks for) holds the Winograd route's seven right-hand
# planes in chunks of >= 8192 paired rows -- two chunks here (10496 + 9504)
@pytest.fixture(scope="module")
def prob(P):
    return _problem(P, 40000, 512, 2048)


def test_route_against_the_oracle(P, prob):
    """The Gaussian/identity cost through the Winograd route against the step written out in fp64 on the CPU."""
    gb, y, fstar, g, u = prob
    gc = P.costs.GaussianCost(0.3, y, P.links.IdentityLinkFunction())
    xi = torch.randn(u.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    eta = 1e-3
    assert probe_winograd(P, gb, gc, u)
    got = gb.fused_step(gc, u, eta, noise=P.basis.NoiseSpec(injected=xi.cuda()), force_generic=True).cpu()
    a, lam, uc = gb._A.cpu(), gb.eigenvalues.cpu(), u.cpu()
    drift = a @ ((a.T @ uc - y[:, None]) / 0.3) + uc / lam[:, None]
    want = -eta * drift + (2 * eta) ** 0.5 * xi
    assert relerr(got, want) < TOL
    assert row_relerr(got, want) < TOL


@pytest.mark.parametrize("energies", [False, True])
def test_every_cost_matches_the_plain_route(P, prob, energies):
    gb, y, fstar, g, u = prob
    j = u.shape[1]
    for name, _, gc in make_costs(P, y, fstar, torch.Generator().manual_seed(5)):
        if not gc.is_native():
            continue
        ns = P.basis.NoiseSpec(seed=11, step=3)

        def run():
            e = torch.full((j,), float("nan"), dtype=torch.float64, device="cuda") if energies else None
            out = gb.fused_step(gc, u, 1e-3, noise=ns, force_generic=True, input_energy=e)
            return out, e

        assert probe_winograd(P, gb, gc, u, eta=1e-3, energy=torch.empty(j, device="cuda") if energies else None), name
        (plain, ep), (wino, ew) = _both_routes(P, run)
        assert torch.isfinite(wino).all(), name
        assert relerr(wino, plain) < 1e-12, name
        assert row_relerr(wino, plain) < 1e-10, name
        if energies:
            assert torch.isfinite(ew).all(), name
            assert relerr(ew, ep) < 1e-12, name


def test_blocks_and_shard_offset(P, prob):
    gb, y, fstar, g, u = prob
    j = u.shape[1]
    gc = P.costs.BernoulliCost((y > 0).double(), P.links.SigmoidLinkFunction())
    eta = torch.tensor([1e-3, 0.0, 2e-3, 5e-4], dtype=torch.float64, device="cuda")
    blocks = P.basis.BlockSpec(j // 4, eta)
    ns = P.basis.NoiseSpec(seed=7, step=2, j_offset=4096)
    assert probe_winograd(P, gb, gc, u, blocks=blocks, noise=ns, new_state=True)
    plain, wino = _both_routes(P, lambda: gb.fused_step(gc, u, 0.0, noise=ns, force_generic=True, blocks=blocks, new_state=True))
    assert relerr(wino, plain) < 1e-12
    frozen = slice(j // 4, j // 2)  # block of step size 0: the particles stay, bit for bit
    assert torch.equal(wino[:, frozen], u[:, frozen])


def test_several_chunks_and_injected_noise(P, prob):
    gb, y, fstar, g, u = prob
    lib = P.pkg._lib.load()
    yc = torch.poisson((2.0 * fstar) ** 2 + 0.5, generator=g)
    gc = P.costs.PoissonCost(yc, P.links.SquareLinkFunction())
    xi = torch.randn(u.shape, generator=g, dtype=torch.float64).cuda()
    ns = P.basis.NoiseSpec(injected=xi)
    j = u.shape[1]
    saved = gb.workspace_bytes
    # 9/10 of the plain route's all-rows workspace: the 20000 paired rows stream in three chunks (9216 + 9216 + 1568), and
    # the energies go through column_reduce's first / accumulate / finish passes
    gb.workspace_bytes = 9 * lib.pls_onb_step_workspace_bytes(gb._desc(), j, 0) // 10
    gb._ws.clear()

    def run():
        e = torch.full((j,), float("nan"), dtype=torch.float64, device="cuda")
        return gb.fused_step(gc, u, 1e-4, noise=ns, force_generic=True, input_energy=e), e

    try:
        assert probe_winograd(P, gb, gc, u, eta=1e-4, energy=torch.empty(j, device="cuda"))
        (plain, ep), (chunked, ec) = _both_routes(P, run)
    finally:
        gb.workspace_bytes = saved
        gb._ws.clear()
    assert relerr(chunked, plain) < 1e-12
    assert torch.isfinite(ec).all()
    assert relerr(ec, ep) < 1e-12
    # ... and against the energies written out in fp64 on the host (cost_j(F) + 1/2 sum_m U_mj^2 / lam_m), on a column sample
    cols = spread_columns(j)
    a, lam, uc = gb._A.cpu(), gb.eigenvalues.cpu(), u.cpu()[:, cols]
    f = a.T @ uc
    want = (-2.0 * yc[:, None] * torch.log(f.abs()) + f * f).sum(0) + 0.5 * (uc * uc / lam[:, None]).sum(0)
    assert ((ec.cpu()[cols] - want).abs() / want.abs()).max().item() < 1e-12


@pytest.mark.parametrize("shape", [(40000, 512, 2000), (40002, 512, 2048), (40000, 504, 2048)])
def test_shapes_outside_the_route_are_unchanged(P, shape):
    n, mk, j = shape
    gb, y, fstar, g, u = _problem(P, n, mk, j, seed=2)
    gc = P.costs.GaussianCost(0.3, y, P.links.IdentityLinkFunction())
    ns = P.basis.NoiseSpec(seed=1, step=1)
    plain, same = _both_routes(P, lambda: gb.fused_step(gc, u, 1e-3, noise=ns, force_generic=True))
    assert torch.equal(plain, same)


# ---- the route's envelope, exactly -------------------------------------------------------------------------------------------
def _host_step(a, lam, u, y, cost, eta):
    """the step of the Gaussian (variance 0.3) or the Bernoulli/sigmoid cost written out in fp64, no noise"""
    f = a.T @ u
    if cost == "gaussian":
        g = (f - y[:, None]) / 0.3
    else:
        p = torch.sigmoid(f).clamp(1e-10, 1 - 1e-10)
        yy = (y > 0).double()[:, None]
        g = -yy * (1 - p) + (1 - yy) * p
    return -eta * (a @ g) - eta * u / lam[:, None]


@pytest.mark.parametrize("shape", WINO_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_envelope_shapes(P, shape):
    """Each shape in a workspace for all paired rows: the probe sees the route; exact problems give the exact step on both
    routes (blocks across J/2, one frozen, a strided particle matrix and output, energies); on real-valued data Gaussian and
    Bernoulli/sigmoid match the host step per eigen-direction."""
    mk, n, j = shape
    ws = wino_one_chunk_bytes(mk, n, j)
    ex = ExactProblem(mk, n, j, seed=n + mk + j)
    gb, cost = ex.basis(P), ex.cost(P)
    planes = gb._winograd_planes(gb._desc())
    assert planes is not None
    cols = torch.unique(torch.cat([spread_columns(j), torch.tensor([j - 1])]))
    want, e_want = ex.step(cols, noise=True, new_state=True)
    # a particle matrix and an output viewed out of wider, aligned buffers (ldu, ldo = J + 128); guard columns of NaN
    wide_u = torch.full((mk, j + 128), float("nan"), device="cuda")
    wide_u[:, :j] = ex.u.cuda()
    u = wide_u[:, :j]
    assert probe_winograd(P, gb, cost, u, ws_bytes=ws)
    xi = P.basis.NoiseSpec(injected=ex.xi.cuda())
    outs = {}
    for mode in (1, 0):
        with winograd_option(P, mode):
            wide_o = torch.full((mk, j + 128), float("nan"), device="cuda")
            e = torch.full((j,), float("nan"), device="cuda")
            step_wg(P, gb, cost, u, EXACT_ETA, planes, noise=xi, out=wide_o[:, :j], new_state=True, energy=e, ws_bytes=ws)
            assert wide_o[:, j:].isnan().all(), f"route {mode} wrote past J"
            got = wide_o[:, :j].cpu()
            assert torch.equal(got[:, cols], want), f"route {mode}: {(got[:, cols] - want).abs().max().item():.3e}"
            assert ((e.cpu()[cols] - e_want).abs() / e_want.abs()).max().item() <= 1e-13
            outs[mode] = got
    assert torch.equal(outs[0], outs[1])
    # per-block step sizes: blocks of 3/8 J straddle J/2, the second one frozen
    bc = 3 * j // 8
    etas = [EXACT_ETA, 0.0, 4 * EXACT_ETA]
    blocks = P.basis.BlockSpec(bc, torch.tensor(etas, device="cuda"))
    got = step_wg(P, gb, cost, u, 0.0, planes, noise=xi, blocks=blocks, ws_bytes=ws).cpu()
    want_b, _ = ex.step(cols, eta=torch.tensor(etas)[cols // bc])
    assert torch.equal(got[:, cols], want_b)
    assert (got[:, bc:2 * bc] == 0).all()
    # Philox noise at a J-shard offset off the 128 grid: the drift is exact, the noise the same pairs -> the same bits
    ns = P.basis.NoiseSpec(seed=3, step=5, j_offset=4100)
    wino = step_wg(P, gb, cost, u, EXACT_ETA, planes, noise=ns, ws_bytes=ws)
    with winograd_option(P, 0):
        plain = step_wg(P, gb, cost, u, EXACT_ETA, planes, noise=ns, ws_bytes=ws)
    assert torch.equal(wino, plain)
    del gb, planes, wide_u, wide_o, outs
    # real-valued operands: per eigen-direction against the host step
    gb, y, fstar, g, u = _problem(P, n, mk, j, seed=n + mk)
    a, lam = gb._A.cpu(), gb.eigenvalues.cpu()
    planes = gb._winograd_planes(gb._desc())
    for name, gc in (("gaussian", P.costs.GaussianCost(0.3, y, P.links.IdentityLinkFunction())),
                     ("bernoulli", P.costs.BernoulliCost((y > 0).double(), P.links.SigmoidLinkFunction()))):
        got = step_wg(P, gb, gc, u, 1e-3, planes, ws_bytes=ws).cpu()[:, cols]
        want = _host_step(a, lam, u.cpu()[:, cols], y, name, 1e-3)
        assert row_relerr(got, want) < TOL, name


def test_three_chunks_exactly(P):
    """three chunks of paired rows, the last one short, several slabs: the products accumulate onto the previous chunks'
    (beta 1), the energies through column_reduce's first / accumulate / finish passes"""
    mk, n, j = WINO_THREE_CHUNKS
    ex = ExactProblem(mk, n, j, seed=11)
    gb, cost = ex.basis(P), ex.cost(P)
    gb.workspace_bytes = 9 * P.pkg._lib.load().pls_onb_step_workspace_bytes(gb._desc(), j, 0) // 10
    u = ex.u.cuda()
    assert probe_winograd(P, gb, cost, u, energy=torch.empty(j, device="cuda"))
    cols = spread_columns(j)
    want, e_want = ex.step(cols)
    for mode in (1, 0):
        with winograd_option(P, mode):
            e = torch.full((j,), float("nan"), device="cuda")
            got = gb.fused_step(cost, u, EXACT_ETA, noise=P.basis.NoiseSpec(injected=ex.xi.cuda()), force_generic=True,
                                input_energy=e)
        assert torch.equal(got.cpu()[:, cols], want), mode
        assert ((e.cpu()[cols] - e_want).abs() / e_want.abs()).max().item() <= 1e-13, mode


@pytest.mark.parametrize("shape", WINO_OUTSIDE + ["u+1"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_just_outside_the_route(P, shape):
    """M_k = 496, N = 16380, J = 1920, J = 2112, a particle matrix one column into its buffer (8-byte aligned): even with
    left-hand planes handed in and room for one chunk, the planes are never read and the step is the plain route's"""
    mk, n, j = (512, 16384, 2048) if shape == "u+1" else shape
    ex = ExactProblem(mk, n, j, seed=mk + n + j)
    gb, cost = ex.basis(P), ex.cost(P)
    if shape == "u+1":
        wide = torch.zeros((mk, j + 128), device="cuda")
        wide[:, 1:j + 1] = ex.u.cuda()
        u = wide[:, 1:j + 1]
    else:
        u = ex.u.cuda()
    assert not probe_winograd(P, gb, cost, u, ws_bytes=wino_one_chunk_bytes(mk, n, j))
    assert not probe_winograd(P, gb, cost, u)


# ---- a graded spectrum at the headline shape ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ls_scale", [1.0, 3.0])
def test_graded_spectrum_per_direction(P, ls_scale, capsys):
    """configs[1]'s data at N = 1e5, J = 8192 (length scales as benched, and x3: lambda spans ~11 decades), threshold 0, M_k
    trimmed to a multiple of 16, the bench's 8 GiB workspace.  The rows of A scale like sqrt(lambda), so relerr over the whole
    matrix cannot see a wrong small direction.  Every route's step per eigen-direction within TOL; then D = A G alone (the basis
    rebuilt with lambda = 2^1000, so the prior term vanishes and D = -step / eta exactly): the plain route per row within
    1e-12, Winograd within 10x the host emulation of the same combination on the same columns (+ 1e-14)."""
    cfg = bench.CONFIGS["c2"]
    x, z, y, ls = bench.make_data(cfg)
    kern = P.pkg.PLSKernel(P.pkg.ARDKernel(ls * ls_scale, 1.0), z)
    gb = P.basis.OrthonormalBasis(kern, z, x, 0.0, verbose=False, keep_gram=False)
    lam_all, vec_all = torch.linalg.eigh((1 / z.shape[0]) * gb.base_gram_induce.cpu())
    keep = torch.where(lam_all > 0)[0]
    keep = keep[keep.numel() % 16:]  # (the smallest go)
    gb = P.basis.OrthonormalBasis(kern, z, x, 0.0, spectrum=(lam_all[keep], vec_all[:, keep]), verbose=False, keep_gram=False)
    mk, j, n = gb.approximation_dimension, cfg["j"], cfg["n"]
    assert mk % 16 == 0 and mk >= 512
    gb.workspace_bytes = 8 << 30
    lam = gb.eigenvalues.cpu()
    u = torch.randn(mk, j, generator=torch.Generator().manual_seed(1)) * lam.sqrt()[:, None]
    ud = u.cuda()
    gc = P.costs.GaussianCost(cfg["obs"], y, P.links.IdentityLinkFunction())
    eta = 2.0 ** -17
    none = P.basis.NoiseSpec(none=True)
    cols = spread_columns(j, per_tile=0)
    a = gb._A.cpu()
    us = u[:, cols]
    gs = (a.T @ us - y[:, None]) / cfg["obs"]
    d_ref = a @ gs
    step_ref = -eta * d_ref - eta * us / lam[:, None]
    assert probe_winograd(P, gb, gc, ud, eta=eta)
    steps = {"winograd": gb.fused_step(gc, ud, eta, noise=none, force_generic=True),
             "fast path": gb.fused_step(gc, ud, eta, noise=none)}
    with winograd_option(P, 0):
        steps["plain"] = gb.fused_step(gc, ud, eta, noise=none, force_generic=True)
    for name, s in steps.items():
        assert row_relerr(s.cpu()[:, cols], step_ref) <= TOL, name
    del steps, gb
    gd = P.basis.OrthonormalBasis.from_projection(a.cuda(), torch.full((mk,), 2.0 ** 1000).cuda())
    gd.workspace_bytes = 8 << 30
    assert probe_winograd(P, gd, gc, ud, eta=eta)
    d_wino = -gd.fused_step(gc, ud, eta, noise=none, force_generic=True).cpu()[:, cols] / eta
    with winograd_option(P, 0):
        d_plain = -gd.fused_step(gc, ud, eta, noise=none, force_generic=True).cpu()[:, cols] / eta
    emu = torch.from_numpy(_winograd(a.numpy(), gs.numpy()))
    e_plain, e_wino, e_emu = row_relerr(d_plain, d_ref), row_relerr(d_wino, d_ref), row_relerr(emu, d_ref)
    with capsys.disabled():
        print(f"\n[graded spectrum ls x{ls_scale:g}: M_k {mk}, lambda {lam.min().item():.1e} .. {lam.max().item():.1e}] per-row error"
              f" of D: plain {e_plain:.2e}, Winograd {e_wino:.2e}, host emulation {e_emu:.2e}")
    assert e_plain <= 1e-12
    assert e_wino <= 10 * e_emu + 1e-14
