"""CPU: the host side of exact-GP hyper-parameter learning -- the LAPACK yardstick against 50-digit arithmetic, the
softplus chain rule against autograd, the training loop's stop rule, the two averaging rules, the nearest-neighbour
subsample, and the argument checks of the two new C-ABI entry points (they run before any HIP call)."""
import math

import numpy as np
import pytest
import torch

import exact_gp_truth as T
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd.gaussian_process import NOISE_LOWER_BOUND

L = pkg._lib
F64 = torch.float64
softplus = torch.nn.functional.softplus


def test_the_case_table_is_the_issue_s():
    sizes = {(n, d) for _, n, d, _ in T.CASES.values()}
    assert sizes == {(n, d) for n in (1, 2, 65, 130, 260) for d in (1, 3, 8)}
    for n, d in sizes:
        kinds = {k for k, nn, dd, _ in T.CASES.values() if (nn, dd) == (n, d)}
        assert kinds == (set(T.KINDS) if n == 65 else {T.RBF, T.MATERN52})


@pytest.mark.parametrize("name", list(T.CASES))
def test_lapack_yardstick_against_50_digits(name):
    """e_cpu: the error of the float64 LAPACK evaluation per output, relative to the output's sum of magnitudes S.  Bound:
    the forward error of a backward-stable solve / inverse, cond(K_y) eps with cond <= 2e3 on these cases (the terms of S
    bound every product that enters an output), 4.4e-13; the GPU tests take their bar from the measured e_cpu."""
    kind, x, y, ls = T.case_inputs(name)
    _, mag, e_cpu = T.cpu_case(name)
    n = x.shape[0]
    cond = torch.linalg.cond(T.OUTPUTSCALE * T.kappa(kind, x, ls) + T.NOISE * torch.eye(n, dtype=F64)).item()
    print(f"{name}: cond {cond:.1e}  e_cpu " + " ".join(f"{v:.1e}" for v in e_cpu))
    assert cond <= 2e3
    assert np.all(e_cpu <= 2e3 * T.EPS), e_cpu


def _autograd_loss(kind, x, y, raw, ard):
    """-mll / n as a differentiable function of the raw parameters (torch autograd through LAPACK)"""
    n, d = x.shape
    mean, noise, s = raw[0], NOISE_LOWER_BOUND + softplus(raw[1]), softplus(raw[2])
    ls = softplus(raw[3:]).expand(d)
    e2 = ((x[:, None, :] - x[None, :, :]) / ls).square().sum(-1)
    if kind == T.RBF:
        kap = torch.exp(-0.5 * e2)
    else:  # Matern-5/2; sqrt has no derivative at 0: the diagonal is taken out before it
        off = ~torch.eye(n, dtype=torch.bool)
        t = torch.sqrt(5.0 * torch.where(off, e2, torch.ones_like(e2)))
        kap = torch.where(off, (1.0 + t + t * t / 3.0) * torch.exp(-t), torch.ones_like(e2))
    low = torch.linalg.cholesky(s * kap + noise * torch.eye(n, dtype=F64))
    r = y - mean
    alpha = torch.cholesky_solve(r[:, None], low)[:, 0]
    mll = -0.5 * r @ alpha - torch.log(low.diagonal()).sum() - 0.5 * n * math.log(2.0 * math.pi)
    return -mll / n


@pytest.mark.parametrize("kernel,kind", [("rbf", T.RBF), ("matern52", T.MATERN52)])
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_against_autograd(kernel, kind, ard):
    g = torch.Generator().manual_seed(40 + kind + ard)
    n, d = 30, 3
    x, y = torch.randn(n, d, generator=g, dtype=F64), torch.randn(n, generator=g, dtype=F64)
    model = pkg.ExactGP(x, y, kernel, ard=ard)
    assert model.raw_parameters().tolist() == [0.0] * (3 + (d if ard else 1))  # every raw value starts at 0
    assert model.lengthscale.tolist() == [math.log(2.0)] * d and model.noise == 1e-4 + math.log(2.0)
    raw = torch.randn(3 + (d if ard else 1), generator=g, dtype=F64) * 0.5
    model.set_raw_parameters(raw)
    loss, grad = T.host_evaluate(model)
    leaf = raw.clone().requires_grad_(True)
    want = _autograd_loss(kind, x, y, leaf, ard)
    want.backward()
    assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
    assert (grad - leaf.grad).abs().max().item() <= 1e-11 * leaf.grad.abs().max().item()
    k = model.kernel
    assert type(k) is (pkg.ARDKernel if kind == T.RBF else pkg.MaternKernel) and k.kind == kind
    assert torch.equal(k.lengthscale, softplus(raw[3:]).expand(d)) and k.outputscale == softplus(raw[2]).item()
    assert model.mean_constant == raw[0].item() and model.noise == 1e-4 + softplus(raw[1]).item()


def _data(n=40, d=2, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.sin(x[:, 0]) + 0.1 * torch.randn(n, generator=g, dtype=F64)


def test_training_loop_on_the_host_yardstick():
    x, y = _data()
    args = dict(seed=1, number_of_epochs=25, learning_rate=0.05, early_stopper_patience=10.0, evaluate=T.host_evaluate)
    model, losses = pkg.train_exact_gp(x, y, "rbf", **args)
    assert len(losses) == 25 and all(b < a for a, b in zip(losses, losses[1:])), losses
    again, losses2 = pkg.train_exact_gp(x, y, "rbf", **args)
    assert losses2 == losses and torch.equal(again.raw_parameters(), model.raw_parameters())
    assert pkg.train_exact_gp(x, y, pkg.MaternKernel([0.5, 2.0], 1.5, nu=1.5), **args)[0].kind == T.MATERN32


def test_stop_rule_is_checked_before_the_loss_is_kept_and_before_the_step():
    """trainers.py:45-50 of the reference: a non-finite or stale loss ends the loop un-appended and un-stepped"""
    x, y = _data()
    calls, seen = [], []

    def nan_on_fourth(model):
        calls.append(1)
        seen.append(model.raw_parameters())
        loss, grad = T.host_evaluate(model)
        return (float("nan") if len(calls) == 4 else loss), grad

    model, losses = pkg.train_exact_gp(x, y, "rbf", 1, 10, 0.05, 10.0, evaluate=nan_on_fourth)
    assert len(calls) == 4 and len(losses) == 3
    assert torch.equal(model.raw_parameters(), seen[3]) and not torch.equal(seen[3], seen[2])  # no step after the stop
    calls.clear()

    def constant(model):
        calls.append(1)
        return 1.25, torch.ones(model.raw.numel(), dtype=F64)

    # the second loss does not improve: 0.05 of simulated time without improvement reaches the patience
    model, losses = pkg.train_exact_gp(x, y, "rbf", 1, 10, 0.05, 0.05, evaluate=constant)
    assert losses == [1.25] and len(calls) == 2
    calls.clear()
    model, losses = pkg.train_exact_gp(x, y, "rbf", 1, 10, 0.05, 0.1, evaluate=constant)
    assert losses == [1.25, 1.25] and len(calls) == 3


def test_the_two_averaging_rules():
    """the kernel averages RAW parameters (then softplus), the noise averages the noises themselves"""
    x, y = _data(10, 2)
    a = pkg.ExactGP(x, y, "matern32").set_raw_parameters(torch.tensor([0.3, -2.0, 1.0, -1.0, 2.0], dtype=F64))
    b = pkg.ExactGP(x, y, "matern32").set_raw_parameters(torch.tensor([0.1, 1.0, -3.0, 3.0, -1.0], dtype=F64))
    k = pkg.construct_average_ard_kernel([a, b])
    assert type(k) is pkg.MaternKernel and k.nu == 1.5
    assert torch.equal(k.lengthscale, softplus(torch.tensor([1.0, 0.5], dtype=F64)))
    assert k.outputscale == softplus(torch.tensor(-1.0, dtype=F64)).item()
    natural = 0.5 * (a.lengthscale + b.lengthscale)
    assert (k.lengthscale - natural).abs().min().item() > 0.05  # (not the average of the natural values)
    noise = pkg.construct_average_gaussian_noise([a, b])
    assert noise == pytest.approx(0.5 * (a.noise + b.noise), rel=1e-15)
    assert abs(noise - (1e-4 + softplus(torch.tensor(-0.5, dtype=F64)).item())) > 0.05  # (not the noise of the averaged raw value)
    assert type(pkg.construct_average_ard_kernel([pkg.ExactGP(x, y, "rbf")])) is pkg.ARDKernel


def test_nearest_subsample_against_a_brute_force_sort():
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(300, 4, generator=g, dtype=F64), torch.randn(300, generator=g, dtype=F64)
    centre = x[17:18]
    xs, ys = pkg.nearest_subsample(x, y, 50, centre)
    order = sorted(range(300), key=lambda i: float(((x[i] - centre[0]) ** 2).sum()))[:50]
    assert torch.equal(xs, x[order]) and torch.equal(ys, y[order]) and order[0] == 17
    xs, ys = pkg.nearest_subsample(x, y, 301, centre)
    assert xs is x and ys is y


def test_cabi_argument_checks_run_before_any_hip_call():
    lib = L.load()
    p = 16  # any non-NULL address: nothing is dereferenced before the checks pass

    def sums(kind=0, x=p, n=4, d=2, ls=p, alpha=p, P=p, ldp=4, out=p, ws=p, nbytes=1 << 20):
        return lib.pls_kernel_grad_sums(kind, x, n, d, ls, 1.0, alpha, P, ldp, out, ws, nbytes, None), lib.pls_last_error()

    def mll(kind=0, x=p, n=4, d=2, ls=p, noise=0.1, jitter=0.0, y=p, out=p, info=p, ws=p, nbytes=1 << 20):
        return lib.pls_gp_mll_grad(kind, x, n, d, ls, 1.0, noise, 0.0, jitter, y, out, info, ws, nbytes, None), lib.pls_last_error()

    for call in (sums, mll):
        assert call(kind=5)[0] == 1 and b"unknown kernel kind 5" in call(kind=5)[1]
        assert call(kind=-1)[0] == 1 and b"unknown kernel kind" in call(kind=-1)[1]
        assert call(kind=L.KERNEL_LINEAR)[0] == 1 and b"linear kernel" in call(kind=L.KERNEL_LINEAR)[1]
        for bad in (dict(n=0), dict(n=-3), dict(d=0), dict(d=-1)):
            assert call(**bad)[0] == 1 and b"bad sizes" in call(**bad)[1], bad
        assert call(d=65)[0] == 1 and b"> 64 is not supported" in call(d=65)[1]
        assert call(ws=None)[0] == 1 and b"NULL workspace" in call(ws=None)[1]
        rc, msg = call(nbytes=8)
        assert rc == 3 and b"workspace of 8 bytes" in msg, msg
    for name in ("x", "ls", "alpha", "P", "out"):
        assert sums(**{name: None})[0] == 1 and b"NULL pointer" in sums(**{name: None})[1], name
    assert sums(ldp=3)[0] == 1 and b"ldp < n" in sums(ldp=3)[1]
    for name in ("x", "ls", "y", "out", "info"):
        assert mll(**{name: None})[0] == 1 and b"NULL pointer" in mll(**{name: None})[1], name
    assert mll(noise=-1e-9)[0] == 1 and b"noise must be >= 0" in mll(noise=-1e-9)[1]
    assert mll(noise=float("nan"))[0] == 1 and mll(jitter=-1.0)[0] == 1 and b"jitter" in mll(jitter=-1.0)[1]
    assert mll(ws=24)[0] == 1 and b"16-byte aligned" in mll(ws=24)[1]
    # the documented workspace formulas
    assert lib.pls_kernel_grad_sums_workspace_bytes(515, 5) == 8 * 6 * 2 * 9
    assert lib.pls_gp_mll_workspace_bytes(5, 3) == 8 * (7 * 5 * 6 + 2 * 6 + 4 + 4)
    assert lib.pls_gp_mll_workspace_bytes(0, 3) == 0 and lib.pls_kernel_grad_sums_workspace_bytes(4, 65) == 0
    assert lib.pls_gp_mll_workspace_bytes(5000, 8) <= 8 * 8 * 5000 * 5000


def test_kernel_argument_of_exact_gp():
    x, y = _data(10, 2)
    assert pkg.ExactGP(x, y, "matern", nu=0.5).kind == T.MATERN12 and pkg.ExactGP(x, y, "matern").kind == T.MATERN52
    with pytest.raises(ValueError):
        pkg.ExactGP(x, y, "linear")
    with pytest.raises(ValueError, match="nu"):
        pkg.ExactGP(x, y, "matern", nu=2.0)
    with pytest.raises(TypeError):
        pkg.ExactGP(x, y, pkg.LinearKernel())
    started = pkg.ExactGP(x, y, pkg.ARDKernel([0.5, 2.0], 1.5))
    assert torch.allclose(started.lengthscale, torch.tensor([0.5, 2.0], dtype=F64), rtol=1e-14) and abs(started.outputscale - 1.5) < 1e-14
