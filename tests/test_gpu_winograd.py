"""GPU: the Strassen-Winograd route of the orthonormal basis' general step (csrc/winograd.h, PLS_OPT_WINOGRAD) against the plain
route on the same inputs: every cost/link pair with and without the energy by-product, per-block step sizes, a J-shard's
j_offset, N streamed in several chunks of paired rows, and shapes outside the route, which must not move a bit."""
import pytest
import torch

from test_gpu_parity import TOL, P, _f64_default, make_costs, relerr  # noqa: F401

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
    got = gb.fused_step(gc, u, eta, noise=P.basis.NoiseSpec(injected=xi.cuda()), force_generic=True).cpu()
    a, lam, uc = gb._A.cpu(), gb.eigenvalues.cpu(), u.cpu()
    drift = a @ ((a.T @ uc - y[:, None]) / 0.3) + uc / lam[:, None]
    want = -eta * drift + (2 * eta) ** 0.5 * xi
    assert relerr(got, want) < TOL


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

        (plain, ep), (wino, ew) = _both_routes(P, run)
        assert torch.isfinite(wino).all(), name
        assert not torch.equal(plain, wino), f"{name}: the Winograd route was not taken"
        assert relerr(wino, plain) < 1e-12, name
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
    plain, wino = _both_routes(P, lambda: gb.fused_step(gc, u, 0.0, noise=ns, force_generic=True, blocks=blocks, new_state=True))
    assert not torch.equal(plain, wino)
    assert relerr(wino, plain) < 1e-12
    frozen = slice(j // 4, j // 2)  # block of step size 0: the particles stay, bit for bit
    assert torch.equal(wino[:, frozen], u[:, frozen])


def test_several_chunks_and_injected_noise(P, prob):
    gb, y, fstar, g, u = prob
    lib = P.pkg._lib.load()
    gc = P.costs.PoissonCost(torch.poisson((2.0 * fstar) ** 2 + 0.5, generator=g), P.links.SquareLinkFunction())
    xi = torch.randn(u.shape, generator=g, dtype=torch.float64).cuda()
    ns = P.basis.NoiseSpec(injected=xi)
    e = torch.empty(u.shape[1], dtype=torch.float64, device="cuda")
    saved = gb.workspace_bytes
    # 9/10 of the plain route's all-rows workspace: the 20000 paired rows stream in three chunks (9216 + 9216 + 1568)
    gb.workspace_bytes = 9 * lib.pls_onb_step_workspace_bytes(gb._desc(), u.shape[1], 0) // 10
    gb._ws.clear()
    try:
        plain, chunked = _both_routes(P, lambda: gb.fused_step(gc, u, 1e-4, noise=ns, force_generic=True, input_energy=e))
    finally:
        gb.workspace_bytes = saved
        gb._ws.clear()
    assert not torch.equal(plain, chunked)
    assert relerr(chunked, plain) < 1e-12


@pytest.mark.parametrize("shape", [(40000, 512, 2000), (40002, 512, 2048), (40000, 504, 2048)])
def test_shapes_outside_the_route_are_unchanged(P, shape):
    n, mk, j = shape
    gb, y, fstar, g, u = _problem(P, n, mk, j, seed=2)
    gc = P.costs.GaussianCost(0.3, y, P.links.IdentityLinkFunction())
    ns = P.basis.NoiseSpec(seed=1, step=1)
    plain, same = _both_routes(P, lambda: gb.fused_step(gc, u, 1e-3, noise=ns, force_generic=True))
    assert torch.equal(plain, same)
