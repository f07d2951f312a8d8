"""CPU: the exact problems of the inducing-point basis (step_fixtures.ExactIpbProblem) are exact on the host alone, for every
shape tests/test_gpu_exact_ipb.py runs.  LAPACK's blocked Cholesky reproduces the constructed factor and its solve the
constructed solution bit for bit, the explicit inverse is Lc^-T Lc^-1 bit for bit, and every step -- original and whitened
coordinates, per-block step sizes, three consecutive whitened steps -- comes out the same with the contraction index of
every product reversed.  With the bit budget the constructor asserts from the data (_bound), that is the proof that a bit
of difference on the GPU is the kernel's."""
import pytest
import torch

from step_fixtures import BLOCK_ETAS, ExactIpbProblem, _unit, exact_ipb_cases


@pytest.fixture(autouse=True)
def _f64_default():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(prev)


def test_unit_is_the_finest_bit():
    assert _unit(torch.tensor([6.0, -20.0, 0.0])) == 2.0
    assert _unit(torch.tensor([0.375, 3.0])) == 0.125
    assert _unit(torch.tensor([2.0 ** 40 + 2.0 ** -12])) == 2.0 ** -12
    assert _unit(torch.zeros(3)) == 1.0


def test_the_bit_budget_is_enforced():
    with pytest.raises(AssertionError, match="bits"):
        ExactIpbProblem(64, 300, 40, seed=1, chain=3)  # the default ranges at eta = 2^-21 do not survive a second step


@pytest.mark.parametrize("m,n,j,kw", exact_ipb_cases(), ids=lambda v: str(v) if isinstance(v, int) else ("chain" if v else ""))
def test_the_reference_alone_is_exact(m, n, j, kw):
    ex = ExactIpbProblem(m, n, j, seed=m + n + j, **kw)
    assert (ex.nl @ ex.nl).abs().max() == 0 and torch.equal(ex.nl, torch.tril(ex.nl, -1))
    assert torch.equal(ex.lc @ ex.linv, torch.eye(m)) and torch.equal(ex.linv @ ex.lc, torch.eye(m))
    lc = torch.linalg.cholesky(ex.kzz)
    assert torch.equal(lc, ex.lc), "LAPACK's factor is not the constructed one"
    v = ex.solve(ex.u)
    assert torch.equal(torch.cholesky_solve(ex.u, lc), v), "LAPACK's solve is not the constructed solution"
    assert torch.equal(ex.kzz @ v, ex.u)
    assert torch.equal(torch.cholesky_inverse(lc), ex.linv.T @ ex.linv), "the explicit inverse"
    assert torch.equal(ex.solve(ex.u, reverse=True), v)
    etas = torch.tensor(BLOCK_ETAS)[torch.arange(j) // -(-j // len(BLOCK_ETAS))]
    for step in (ex.step, ex.whitened_step):
        for args in (dict(), dict(new_state=True), dict(noise=False), dict(eta=etas, new_state=True)):
            a, ea = step(**args)
            b, eb = step(reverse=True, **args)
            assert torch.equal(a, b), f"{step.__name__} {args}: the reversed summation differs"
            if ex.energy_exact:
                assert torch.equal(ea, eb)
    # the two coordinate systems describe one step: dU = Lc dS, with the coloured noise e = Lc xi
    du, e_u = ex.step()
    ds, e_s = ex.whitened_step()
    assert torch.equal(ex.lc @ ds, du) and torch.equal(e_u, e_s)
    # ... and the whitened operators give the same dS
    assert torch.equal(-ex.eta * (ex.q @ ex.s - ex.ct) + (2 * ex.eta) ** 0.5 * ex.xi, ds)
    state = back = ex.s
    for k in range(kw.get("chain", 0)):
        xi = ex.chain_noise(k)
        state, _ = ex.whitened_step(new_state=True, state=state, xi=xi)
        back, _ = ex.whitened_step(new_state=True, state=back, xi=xi, reverse=True)
        assert torch.equal(state, back), f"chain step {k}"
