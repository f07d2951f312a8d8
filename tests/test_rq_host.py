"""CPU: the host side of the rational-quadratic base kernel -- the closed-form yardstick against 50-digit arithmetic, the raw
parameter layout of ExactGP / DirichletExactGP with raw alpha as the last column, chain_rule against torch autograd,
gpytorch-shaped objects read by as_base_kernel, the averaging constructor, and the C ABI's argument checks and kind-aware
workspace queries (they run before any HIP call)."""
import math

import numpy as np
import pytest
import torch

import projected_langevin_sampling_amd as pkg
import rq_truth as T
from projected_langevin_sampling_amd.kernel import ARDKernel, MaternKernel, RQKernel, as_base_kernel
from rq_closed_form import ALPHAS, LN2, rq_factors_numpy, rq_numpy, rq_torch

L = pkg._lib
F64 = torch.float64


@pytest.mark.parametrize("k", range(len(ALPHAS)), ids=[f"alpha={a:g}" for a in ALPHAS])
def test_numpy_helper_against_50_digits(k):
    """kappa, g and ga of rq_factors_numpy per pair of the fixture's table.  Bars from the formulas: x = alpha log1p(u) carries
    the roundings of u, of log1p and of the product (3 eps relative), which exp turns into 3 |x| eps; the quotient and the
    products add a few eps (8 allowed).  ga's bracket u / (1 + u) - log1p(u) is summed from its series below u = 0.1 and is
    a plain difference from there on, where its two terms are at most 42 times the result (u = 0.1): 2 * 42 + 8 eps more."""
    alpha = ALPHAS[k]
    hi, lo = T.pair_truth()
    got = rq_factors_numpy(T.PAIR_R2, alpha)
    x = alpha * np.log1p(T.PAIR_R2 / (2.0 * alpha))
    for name, row, extra in (("kappa", 0, 8.0), ("g", 1, 8.0), ("ga", 2, 100.0)):
        want = hi[k, row]
        err = np.abs((got[row] - want) - lo[k, row])
        bar = (3.0 * x + extra) * T.EPS * np.abs(want) + 1e-300  # (the floor: entries that are subnormal or 0)
        print(f"alpha={alpha:g} {name}: max err/bar {np.max(err / bar):.3f}")
        assert np.all(err <= bar), (name, err / bar)
    assert got[0][0] == 1.0 and got[1][0] == 1.0 and got[2][0] == 0.0, "distance 0: kappa = g = 1 and ga = 0 exactly"
    assert np.all(hi[k, 2] <= 0.0), "kappa falls as alpha falls: every ga is <= 0"


def test_closed_forms_agree_and_hold_the_diagonal():
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(7, 3, generator=g, dtype=F64), torch.randn(9, 3, generator=g, dtype=F64)
    ls = 0.5 + torch.rand(3, generator=g, dtype=F64)
    for alpha in ALPHAS:
        a, b = rq_torch(ls, 2.5, alpha)(x1, x2).numpy(), rq_numpy(ls.numpy(), 2.5, alpha)(x1.numpy(), x2.numpy())
        assert np.abs(a - b).max() <= 4 * T.EPS * 2.5
        assert np.all(rq_torch(ls, 2.5, alpha)(x1, x1).diagonal().numpy() == 2.5)
        assert np.all(np.diag(rq_numpy(ls.numpy(), 2.5, alpha)(x1.numpy(), x1.numpy())) == 2.5)
    far = torch.full((1, 3), 1e200, dtype=F64)
    assert rq_torch(ls, 1.0, 3.0)(far, -far).item() == 0.0 and rq_numpy(ls.numpy(), 1.0, 3.0)(far.numpy(), -far.numpy()).item() == 0.0


# ---- kernel objects ------------------------------------------------------------------------------------------------------
def _scale_stub(lengthscale, outputscale, **inner_attributes):
    inner = type("Inner", (), {"lengthscale": lengthscale, **inner_attributes})()
    return type("ScaleStub", (), {"base_kernel": inner, "outputscale": outputscale})()


def test_as_base_kernel_reads_a_scale_rq_kernel():
    k = as_base_kernel(_scale_stub(torch.tensor([[0.5, 2.0, 1.25]]), torch.tensor(3.0), alpha=torch.tensor([0.75])))
    assert type(k) is RQKernel and k.kind == L.KERNEL_RQ == 6
    assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.outputscale == 3.0 and k.alpha == 0.75 and isinstance(k.alpha, float)
    assert k._lengthscale_host(3).tolist() == [0.5, 2.0, 1.25, 0.75], "the library reads alpha behind the d lengthscales"
    k = as_base_kernel(_scale_stub(torch.tensor([[0.75]]), 1.5, alpha=2.0))  # one shared lengthscale, plain floats
    assert type(k) is RQKernel and k.lengthscale.tolist() == [0.75] and k.alpha == 2.0
    assert k._lengthscale_host(4).tolist() == [0.75] * 4 + [2.0]
    assert as_base_kernel(k) is k
    # the nu test comes first: an inner kernel with nu is a Matern kernel whatever else it carries
    m = as_base_kernel(_scale_stub(torch.tensor([[1.0]]), 1.0, nu=1.5, alpha=2.0))
    assert type(m) is MaternKernel and m.nu == 1.5
    assert type(as_base_kernel(_scale_stub(torch.tensor([[1.0]]), 1.0))) is ARDKernel
    assert RQKernel([1.0]).alpha == 1.0 and pkg.RQKernel is RQKernel and "RQKernel" in pkg.__all__
    with pytest.raises(ValueError, match="alpha"):
        RQKernel([1.0], 1.0, alpha=0.0)


# ---- the raw layout ------------------------------------------------------------------------------------------------------
def _data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.sin(x.sum(dim=1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)


def test_exact_gp_raw_layout_and_start_values():
    x, y = _data(12, 3, 1)
    model = pkg.ExactGP(x, y, kernel="rq")
    assert model.kind == L.KERNEL_RQ and model.kernel_name == "rq" and model.raw.shape == (7,)  # 4 + nls
    assert torch.equal(model.raw.detach(), torch.zeros(7, dtype=F64))
    assert model.alpha == pytest.approx(LN2, abs=1e-15) and isinstance(model.alpha, float)
    assert model.lengthscale.shape == (3,) and torch.allclose(model.lengthscale, torch.full((3,), LN2, dtype=F64))
    assert pkg.ExactGP(x, y, kernel="rq", ard=False).raw.shape == (5,)
    start = RQKernel([0.5, 2.0, 1.25], 1.7, alpha=0.3)
    model = pkg.ExactGP(x, y, kernel=start)
    assert model.kind == L.KERNEL_RQ and model.ard and model.raw.shape == (7,)
    assert torch.allclose(model.lengthscale, start.lengthscale, rtol=1e-14)
    assert model.outputscale == pytest.approx(1.7, rel=1e-14) and model.alpha == pytest.approx(0.3, rel=1e-14)
    fitted = model.kernel
    assert type(fitted) is RQKernel and fitted.alpha == model.alpha and fitted.outputscale == model.outputscale
    assert torch.equal(fitted.lengthscale, model.lengthscale)
    shared = pkg.ExactGP(x, y, kernel=RQKernel([0.8], 1.1, alpha=4.0))
    assert not shared.ard and shared.raw.shape == (5,) and shared.alpha == pytest.approx(4.0, rel=1e-14)
    assert torch.allclose(shared.lengthscale, torch.full((3,), 0.8, dtype=F64), rtol=1e-14)
    # round trip; raw alpha is the LAST entry
    raw = torch.tensor([0.1, -1.0, 0.3, 0.2, 0.6, -0.4, 1.5], dtype=F64)
    assert torch.equal(model.set_raw_parameters(raw).raw_parameters(), raw)
    assert model.alpha == pytest.approx(math.log1p(math.exp(1.5)), rel=1e-15)
    assert torch.allclose(model.lengthscale, torch.nn.functional.softplus(raw[3:6]), rtol=1e-15)
    assert model._library_lengthscale().shape == (1, 4) and model._library_lengthscale()[0, 3].item() == model.alpha
    with pytest.raises(AssertionError):
        model.set_raw_parameters(raw[:6])


def test_dirichlet_raw_layout():
    x, _ = _data(12, 2, 2)
    labels = torch.arange(12) % 3
    model = pkg.DirichletExactGP(x, labels, kernel="rq")
    assert model.kind == L.KERNEL_RQ and model.raw.shape == (3, 6) and model.alpha.shape == (3,)
    raw = 0.3 * torch.randn(3, 6, generator=torch.Generator().manual_seed(4), dtype=F64)
    model.set_raw_parameters(raw)
    assert torch.equal(model.raw_parameters(), raw)
    assert torch.allclose(model.alpha, torch.nn.functional.softplus(raw[:, -1]), rtol=1e-15)
    assert torch.allclose(model.lengthscale, torch.nn.functional.softplus(raw[:, 3:5]), rtol=1e-15)
    ls = model._library_lengthscale()
    assert ls.shape == (3, 3) and torch.equal(ls[:, 2], model.alpha) and torch.equal(ls[:, :2], model.lengthscale)
    kernels = model.kernels
    assert [type(k) for k in kernels] == [RQKernel] * 3 and [k.alpha for k in kernels] == model.alpha.tolist()
    one = model.kernel  # the raw values averaged over the classes, softplus afterwards
    assert type(one) is RQKernel and one.alpha == pytest.approx(float(torch.nn.functional.softplus(raw[:, -1].mean())), rel=1e-15)


def test_the_other_layouts_are_unchanged():
    x, y = _data(12, 3, 5)
    for kernel, kind in (("rbf", L.KERNEL_RBF_ARD), ("matern", L.KERNEL_MATERN52), ("matern12", L.KERNEL_MATERN12),
                         ("matern32", L.KERNEL_MATERN32), (ARDKernel([1.0, 2.0, 3.0]), L.KERNEL_RBF_ARD),
                         (MaternKernel([1.0], nu=1.5), L.KERNEL_MATERN32)):
        model = pkg.ExactGP(x, y, kernel=kernel)
        assert model.kind == kind and model.raw.shape == (3 + (3 if model.ard else 1),)
        assert not hasattr(model, "alpha"), "only the rational-quadratic kernel has an alpha"
        out = torch.arange(7, dtype=F64)
        loss, grad = model.chain_rule(out)
        assert grad.shape == model.raw.shape and loss == 0.0
    assert pkg.DirichletExactGP(x, torch.arange(12) % 2, kernel="matern32").raw.shape == (2, 6)
    with pytest.raises(ValueError, match="kernel must be one of"):
        pkg.ExactGP(x, y, kernel="periodic")
    with pytest.raises(TypeError, match="RQKernel"):
        pkg.ExactGP(x, y, kernel=pkg.LinearKernel())


# ---- chain_rule against autograd --------------------------------------------------------------------------------------
def _autograd_loss(x, y, raw, ard):
    """-mll / n of the closed form as a function of the raw parameters (float64, CPU), through torch autograd"""
    n, d = x.shape
    raw = raw.clone().requires_grad_(True)
    sp = torch.nn.functional.softplus
    mean, noise, s, alpha = raw[0], 1e-4 + sp(raw[1]), sp(raw[2]), sp(raw[-1])
    ls = sp(raw[3:-1])
    ls = ls if ard else ls.expand(d)
    r2 = ((x[:, None, :] - x[None, :, :]) / ls).square().sum(-1)
    ky = s * torch.exp(-alpha * torch.log1p(r2 / (2.0 * alpha))) + noise * torch.eye(n, dtype=F64)
    low = torch.linalg.cholesky(ky)
    r = y - mean
    mll = -0.5 * (r * torch.cholesky_solve(r[:, None], low)[:, 0]).sum() - torch.log(low.diagonal()).sum() - 0.5 * n * math.log(2 * math.pi)
    loss = -mll / n
    loss.backward()
    return loss.item(), raw.grad


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_against_autograd(ard):
    """chain_rule fed with the helper's 5 + d outputs gives autograd's loss and raw gradient.  n = 40 points with noise >=
    0.1: cond(K_y) <= 1e3, so two float64 evaluations of a gradient component agree to 1e-13 relative to the largest."""
    x, y = _data(40, 3, 6)
    model = pkg.ExactGP(x, y, kernel="rq", ard=ard)
    g = torch.Generator().manual_seed(7 + ard)
    raw = 0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64)
    raw[1] = -2.0  # noise = 1e-4 + softplus(-2) = 0.127
    model.set_raw_parameters(raw)
    out, _ = T.mll_and_grad(x, y, model.lengthscale, model.alpha, model.outputscale, model.noise, model.mean_constant)
    assert out.shape == (5 + 3,)
    loss, grad = model.chain_rule(torch.from_numpy(out))
    want_loss, want_grad = _autograd_loss(x, y, raw, ard)
    err = ((grad - want_grad).abs().max() / want_grad.abs().max()).item()
    print(f"{'ard' if ard else 'shared'}: loss {loss:.6f} vs {want_loss:.6f}, gradient rel err {err:.2e}, d/d raw alpha {grad[-1]:.3e}")
    assert grad.shape == raw.shape and abs(loss - want_loss) <= 1e-13 * abs(want_loss) and err <= 1e-13
    assert abs(want_grad[-1]) > 1e-4 * want_grad.abs().max(), "test construction: the alpha derivative must matter"
    assert T.host_evaluate(model)[0] == loss


def test_construct_average_ard_kernel_on_two_models():
    x, y = _data(12, 2, 8)
    a, b = pkg.ExactGP(x, y, kernel="rq"), pkg.ExactGP(x, y, kernel="rq")
    a.set_raw_parameters(torch.tensor([0.0, 0.0, 0.2, 0.4, -0.6, 1.0], dtype=F64))
    b.set_raw_parameters(torch.tensor([0.5, 0.1, 0.6, -0.2, 0.2, -2.0], dtype=F64))
    k = pkg.construct_average_ard_kernel([a, b])
    sp = torch.nn.functional.softplus
    assert type(k) is RQKernel
    assert k.alpha == float(sp(torch.tensor(-0.5, dtype=F64))) and k.outputscale == float(sp(torch.tensor(0.4, dtype=F64)))
    assert torch.equal(k.lengthscale, sp(torch.tensor([0.1, -0.2], dtype=F64)))
    shared = pkg.ExactGP(x, y, kernel="rq", ard=False)
    k = pkg.construct_average_ard_kernel([shared])
    assert type(k) is RQKernel and k.lengthscale.numel() == 2 and k.alpha == pytest.approx(LN2, abs=1e-15)


def test_training_loop_and_runner_accept_rq():
    """train_exact_gp and exact_gp_runner with kernel="rq" and with an RQKernel instance, on the host evaluation"""
    x, y = _data(30, 2, 9)
    model, losses = pkg.train_exact_gp(x, y, "rq", seed=1, number_of_epochs=5, learning_rate=0.05, early_stopper_patience=10.0,
                                       evaluate=T.host_evaluate)
    assert model.kind == L.KERNEL_RQ and len(losses) == 5 and losses[-1] < losses[0]
    assert model.raw_parameters()[-1] != 0.0, "raw alpha is learned"
    model, _ = pkg.train_exact_gp(x, y, RQKernel([1.0, 2.0], 1.0, alpha=2.0), seed=1, number_of_epochs=1, learning_rate=0.05,
                                  early_stopper_patience=10.0, evaluate=T.host_evaluate)
    assert model.kind == L.KERNEL_RQ and model.raw.shape == (6,)
    model, _ = pkg.train_exact_gp(x, torch.arange(30) % 2, "rq", seed=1, number_of_epochs=0, learning_rate=0.05,
                                  early_stopper_patience=10.0, likelihood="dirichlet")
    assert type(model) is pkg.DirichletExactGP and model.raw.shape == (2, 6)


# ---- the C ABI (validation only: no HIP call) ---------------------------------------------------------------------------
def test_cabi_accepts_the_kind_and_sizes_its_workspace():
    lib = L.load()
    p = 8  # (any non-NULL address: every call below fails its argument checks first)
    assert lib.pls_abi_version() == L.ABI_VERSION and L.KERNEL_RQ == T.RQ == 6
    assert lib.pls_kernel_gram(L.KERNEL_RQ, p, 1, p, 1, 1, None, 1.0, p, 1, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(L.KERNEL_RQ, p, 4, 1, None, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_kernel_mean(L.KERNEL_RQ, p, 4, 2, None, 1.0, 0.0, p, p, 3, p, None) == 1 and b"NULL pointer" in lib.pls_last_error()
    assert lib.pls_kernel_mean(L.KERNEL_RQ, p, 4, 2, p, 1.0, 0.0, p, p, 0, p, None) == 0
    for kind in (L.KERNEL_RBF_ARD, L.KERNEL_MATERN12, L.KERNEL_MATERN32, L.KERNEL_MATERN52):  # the existing values stay
        for n, d in ((5, 3), (515, 5), (130, 64)):
            assert lib.pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d) == lib.pls_kernel_grad_sums_workspace_bytes(n, d)
            assert lib.pls_gp_mll_workspace_bytes_kind(kind, n, d) == lib.pls_gp_mll_workspace_bytes(n, d)
            assert lib.pls_gp_mll_classes_workspace_bytes_kind(kind, n, d, 3) == lib.pls_gp_mll_classes_workspace_bytes(n, d, 3)
    assert lib.pls_kernel_grad_sums_workspace_bytes(515, 5) == 8 * 6 * 2 * 9
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_RQ, 515, 5) == 8 * 7 * 2 * 9  # d + 2 sums
    assert lib.pls_gp_mll_workspace_bytes(5, 3) == 8 * (7 * 5 * 6 + 2 * 6 + 4 + 4)
    assert lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_RQ, 5, 3) == 8 * (7 * 5 * 6 + 2 * 6 + 6 + 6)  # v(5) = 6 twice
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(L.KERNEL_RQ, 5, 3, 2) == lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_RQ, 5, 3)
    for bad in (L.KERNEL_LINEAR, 5, 7, -1):
        assert lib.pls_gp_mll_workspace_bytes_kind(bad, 5, 3) == 0 and lib.pls_kernel_grad_sums_workspace_bytes_kind(bad, 5, 3) == 0
    assert lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_RQ, 5, 65) == 0 and lib.pls_gp_mll_classes_workspace_bytes_kind(L.KERNEL_RQ, 5, 3, 0) == 0
    # the entries check against the kind-aware need: the old size is one double short for RQ at n = 5, d = 3
    old, need = lib.pls_gp_mll_workspace_bytes(5, 3), lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_RQ, 5, 3)
    assert need > old
    assert lib.pls_gp_mll_grad(L.KERNEL_RQ, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, old, None) == 3  # WORKSPACE_TOO_SMALL
    assert f"{need} needed".encode() in lib.pls_last_error()
    old, need = lib.pls_kernel_grad_sums_workspace_bytes(515, 5), lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_RQ, 515, 5)
    assert lib.pls_kernel_grad_sums(L.KERNEL_RQ, p, 515, 5, p, 1.0, p, p, 515, p, 16, old, None) == 3
    assert f"{need} needed".encode() in lib.pls_last_error()
