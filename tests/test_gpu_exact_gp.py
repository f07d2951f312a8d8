"""GPU: exact-GP hyper-parameter learning -- the kernel-gradient reduction per output against math.fsum of the closed-form
terms (every D_MAX instantiation, both load paths, duplicated and far-apart points), the whole marginal-likelihood
evaluation against 50-digit arithmetic, a matrix that is not positive definite, the training loop against the same loop
on the CPU, prediction, and the hand-over of the fitted kernel and noise to a PLS step."""
import numpy as np
import pytest
import torch

import exact_gp_truth as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
GRAD_DIMS = [1, 2, 3, 5, 8, 13, 33, 64]  # every D_MAX of the reduction: 1, 2, 4, 8, 16, 32, 64, padded and exact
# n = 1: a lone column; 2: a short row block; 65: a second row block of one row; 515: a second column block with an odd tail
GRAD_SHAPES = [(1, 5), (2, 5), (65, 5), (515, 5)] + [(130, d) for d in GRAD_DIMS]


@pytest.fixture(scope="module")
def lib():
    import projected_langevin_sampling_amd as pkg

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return pkg._lib.load()


def _L():
    import projected_langevin_sampling_amd as pkg

    return pkg._lib


def cu(t):
    return t.to(device="cuda", dtype=F64).contiguous()


def grad_sums(lib, kind, x, ls, s, alpha, p_view, ldp):
    """pls_kernel_grad_sums through the C ABI; p_view: a device (n, n) view with leading dimension ldp"""
    L = _L()
    n, d = x.shape
    xd, lsd, ad = cu(x), cu(ls), cu(alpha)
    nbytes = lib.pls_kernel_grad_sums_workspace_bytes(n, d)
    ws = torch.empty(nbytes // 8 + 1, dtype=F64, device="cuda")
    out = torch.full((d + 2,), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_grad_sums(kind, xd.data_ptr(), n, d, lsd.data_ptr(), float(s), ad.data_ptr(), p_view.data_ptr(), ldp,
                                     out.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "pls_kernel_grad_sums")
    host = out.cpu()
    assert torch.isnan(host[d + 1]), "the reduction wrote past its d + 1 outputs"
    return host[: d + 1]


def aligned_copy(p):
    """(device view with an even leading dimension on a 16-byte boundary, ldp)"""
    n = p.shape[0]
    ldp = (n + 1) // 2 * 2
    buf = torch.full((n, ldp), float("nan"), dtype=F64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:, :n] = cu(p)
    return buf, ldp


def reduction_problem(kind, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
    alpha = torch.randn(n, generator=g, dtype=F64)
    a = torch.randn(n, n, generator=g, dtype=F64)
    return x, ls, alpha, a + a.T  # (exactly symmetric; it need not be an inverse)


def check_sums(tag, got, want, scale):
    ratio = np.abs(got.numpy() - want) / np.where(scale > 0, scale, 1.0)
    print(f"{tag}: |got - want| / sum|term| per output, max {ratio.max():.2e}")
    assert np.all(np.isfinite(got.numpy())), (tag, got)
    assert np.all(np.abs(got.numpy() - want) <= 1e-13 * scale), (tag, ratio)


@pytest.mark.parametrize("kind", T.KINDS, ids=[T.KIND_NAMES[k] for k in T.KINDS])
@pytest.mark.parametrize("n,d", GRAD_SHAPES)
def test_reduction_per_output(lib, kind, n, d):
    s = 1.7
    x, ls, alpha, p = reduction_problem(kind, n, d, 7000 + 10 * n + d + kind)
    want, scale = T.grad_sums(kind, x, ls, s, alpha, p)
    buf, ldp = aligned_copy(p)
    got = grad_sums(lib, kind, x, ls, s, alpha, buf, ldp)
    check_sums(f"{T.KIND_NAMES[kind]} n={n} d={d}", got, want, scale)
    assert torch.equal(got, grad_sums(lib, kind, x, ls, s, alpha, buf, ldp)), "two calls differ"
    # odd ldp, 8 bytes past a 16-byte boundary: the scalar load path gives the same bits; the NaN padding is only read around
    ldo = n + 1 + (n % 2)
    raw = torch.full((1 + n * ldo,), float("nan"), dtype=F64, device="cuda")
    view = raw[1:].view(n, ldo)
    assert view.data_ptr() % 16 == 8 and ldo % 2 == 1
    view[:, :n] = cu(p)
    assert torch.equal(got, grad_sums(lib, kind, x, ls, s, alpha, view, ldo)), "scalar load path != 16-byte load path"
    assert torch.isnan(view[:, n:]).all() and torch.isnan(raw[:1]).all() and torch.equal(view[:, :n], cu(p))


@pytest.mark.parametrize("kind", T.KINDS, ids=[T.KIND_NAMES[k] for k in T.KINDS])
def test_reduction_with_duplicated_and_far_points(lib, kind):
    """Pairs at distance 0 (also across column pairs and row blocks) contribute 0 to every lengthscale sum -- nu = 1/2's
    1/t included --, pairs 1e200 apart contribute 0 to every sum; nothing becomes NaN."""
    n, d, s = 130, 5, 1.7
    x, ls, alpha, p = reduction_problem(kind, n, d, 8100 + kind)
    x[10], x[11], x[70], x[129] = x[3], x[3], x[3], x[64]
    buf, ldp = aligned_copy(p)
    want, scale = T.grad_sums(kind, x, ls, s, alpha, p)
    check_sums(f"{T.KIND_NAMES[kind]} duplicates", grad_sums(lib, kind, x, ls, s, alpha, buf, ldp), want, scale)
    x[5], x[6], x[100] = 1e200, 1e200, -1e200
    want, scale = T.grad_sums(kind, x, ls, s, alpha, p)
    assert np.all(np.isfinite(want))
    check_sums(f"{T.KIND_NAMES[kind]} far points", grad_sums(lib, kind, x, ls, s, alpha, buf, ldp), want, scale)


# ---- the whole evaluation ------------------------------------------------------------------------------------------------
def gp_mll(lib, kind, x, y, ls, s, noise, mean, jitter=0.0, fill=None):
    """pls_gp_mll_grad through the C ABI: (the 4 + d outputs on the CPU, info, status)"""
    L = _L()
    n, d = x.shape
    xd, yd, lsd = cu(x), cu(y), cu(ls)
    nbytes = lib.pls_gp_mll_workspace_bytes(n, d)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    if fill is not None:
        ws.fill_(fill)
    out = torch.full((4 + d + 1,), float("nan"), dtype=F64, device="cuda")
    info = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    rc = lib.pls_gp_mll_grad(kind, xd.data_ptr(), n, d, lsd.data_ptr(), float(s), float(noise), float(mean), float(jitter),
                             yd.data_ptr(), out.data_ptr(), info.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr())
    host = out.cpu()
    assert torch.isnan(host[4 + d]), "the evaluation wrote past its 4 + d outputs"
    return host[: 4 + d], int(info.item()), rc


@pytest.mark.parametrize("name", list(T.CASES))
def test_whole_evaluation_against_50_digits(lib, name):
    """Every output against the 50-digit truth, relative to its sum-of-magnitudes scale S.  Bar per output:
    max(16 e_cpu, 64 eps): LAPACK's own error on the case with a margin of 16 for the other association of a blocked
    factorisation, an explicit inverse and MFMA products, and a floor of a few roundings (eps = 2^-52)."""
    kind, x, y, ls = T.case_inputs(name)
    _, mag, e_cpu = T.cpu_case(name)
    hi, lo = T.truth(name)
    got, info, rc = gp_mll(lib, kind, x, y, ls, T.OUTPUTSCALE, T.NOISE, T.MEAN)
    assert rc == 0 and info == 0
    err = T.relative_error(got.numpy(), hi, lo, mag)
    bar = np.maximum(16.0 * e_cpu, 64.0 * T.EPS)
    print(f"{name}: max err/S {err.max():.2e}  max err/bar {np.max(err / bar):.3f}  (e_cpu max {e_cpu.max():.2e})  per output err/bar "
          + " ".join(f"{v:.3f}" for v in err / bar))
    again, _, _ = gp_mll(lib, kind, x, y, ls, T.OUTPUTSCALE, T.NOISE, T.MEAN)
    assert torch.equal(got, again), "two calls differ"
    poisoned, info, rc = gp_mll(lib, kind, x, y, ls, T.OUTPUTSCALE, T.NOISE, T.MEAN, fill=float("nan"))
    assert rc == 0 and info == 0 and torch.equal(got, poisoned), "the result depends on what the workspace held"
    assert np.all(err <= bar), (name, err / bar)


def test_not_positive_definite_is_reported_not_thrown(lib):
    """noise = 0, jitter = 0 and two identical rows: the second pivot is exactly 0 (outputscale 1: sqrt and the quotient
    are exact).  The C ABI reports it in info and returns PLS_OK; the same data through ExactGP (noise >= 1e-4) is fine."""
    import projected_langevin_sampling_amd as pkg

    g = torch.Generator().manual_seed(11)
    x = torch.randn(70, 3, generator=g, dtype=F64)
    x[1] = x[0]
    y = torch.randn(70, generator=g, dtype=F64)
    ls = torch.full((3,), 1.2, dtype=F64)
    for kind in T.KINDS:
        _, info, rc = gp_mll(lib, kind, x, y, ls, 1.0, 0.0, 0.0)
        assert rc == 0 and info == 2, (kind, rc, info)
    loss, grad = pkg.ExactGP(x, y, "rbf").loss_and_grad()
    assert np.isfinite(loss) and torch.isfinite(grad).all()


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
@pytest.mark.parametrize("name", ["rbf-n130-d3", "matern32-n65-d8", "matern52-n2-d1"])
def test_model_evaluation_is_gp_mll_grad(lib, name, ard):
    """ExactGP reaches the device through pls_gp_mll_grad_classes with one class: what it returns is, bit for bit, a
    direct pls_gp_mll_grad call at the model's own parameters, without and with jitter."""
    import projected_langevin_sampling_amd as pkg

    kind, x, y, _ = T.case_inputs(name)
    model = pkg.ExactGP(x, y, T.KIND_NAMES[kind], ard=ard)
    assert model.kind == kind and model.raw.shape == (3 + (x.shape[1] if ard else 1),)
    g = torch.Generator().manual_seed(900 + kind + ard)
    model.set_raw_parameters(0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64))
    for jitter in (0.0, 1e-6):
        out, info = model.evaluate_on_device(jitter)
        want, flag, rc = gp_mll(lib, kind, x, y, model.lengthscale, model.outputscale, model.noise, model.mean_constant, jitter)
        assert rc == 0 and flag == 0 and info == 0
        assert out.shape == (4 + x.shape[1],) and torch.equal(out, want), (name, ard, jitter)


# ---- training ------------------------------------------------------------------------------------------------------------
def _training_data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    y = torch.sin(1.5 * x[:, 0]) + 0.5 * x[:, -1] + 0.2 * torch.randn(n, generator=g, dtype=F64)
    return x, y


@pytest.mark.parametrize("kernel", ["rbf", "matern32"])
def test_training_follows_the_cpu_loop(kernel):
    """train_exact_gp on the library against the same loop with the LAPACK helper as ``evaluate``.  The bar comes from the
    CPU loop alone: rerun with every gradient component perturbed by a relative 1e-12 (alternating signs), 16 x the
    divergence of the losses and of the final raw parameters, floor 1e-11."""
    import projected_langevin_sampling_amd as pkg

    x, y = _training_data(130, 2, 21)
    args = dict(seed=3, number_of_epochs=30, learning_rate=0.05, early_stopper_patience=10.0)

    def perturbed(model):
        loss, grad = T.host_evaluate(model)
        sign = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(grad.numel())], dtype=F64)
        return loss, grad * (1.0 + 1e-12 * sign)

    cpu_model, cpu_losses = pkg.train_exact_gp(x, y, kernel, evaluate=T.host_evaluate, **args)
    per_model, per_losses = pkg.train_exact_gp(x, y, kernel, evaluate=perturbed, **args)
    gpu_model, gpu_losses = pkg.train_exact_gp(x, y, kernel, **args)
    assert len(cpu_losses) == len(per_losses) == len(gpu_losses) == 30
    bar_loss = max(16.0 * np.abs(np.array(cpu_losses) - np.array(per_losses)).max(), 1e-11)
    bar_raw = max(16.0 * (cpu_model.raw_parameters() - per_model.raw_parameters()).abs().max().item(), 1e-11)
    d_loss = np.abs(np.array(cpu_losses) - np.array(gpu_losses)).max()
    d_raw = (cpu_model.raw_parameters() - gpu_model.raw_parameters()).abs().max().item()
    print(f"{kernel}: loss {cpu_losses[0]:.6f} -> {cpu_losses[-1]:.6f}; |gpu - cpu| losses {d_loss:.2e} (bar {bar_loss:.2e}), "
          f"raw {d_raw:.2e} (bar {bar_raw:.2e})")
    assert cpu_losses[-1] < cpu_losses[0] and gpu_losses[-1] < gpu_losses[0]
    assert d_loss <= bar_loss and d_raw <= bar_raw


def test_predict_against_the_helper():
    import projected_langevin_sampling_amd as pkg

    x, y = _training_data(130, 2, 22)
    g = torch.Generator().manual_seed(23)
    xt = torch.randn(40, 2, generator=g, dtype=F64)
    model = pkg.ExactGP(x, y, "matern52")
    model.set_raw_parameters(torch.tensor([0.1, -1.5, 0.3, 0.2, 0.6], dtype=F64))
    s, noise, c, ls = model.outputscale, model.noise, model.mean_constant, model.lengthscale
    from matern_closed_form import matern_torch

    k = matern_torch(ls, s, 2.5)
    ky = k(x, x) + noise * torch.eye(130, dtype=F64)
    assert torch.linalg.cond(ky).item() <= 1e3
    low = torch.linalg.cholesky(ky)
    ks = k(x, xt)
    want_mean = c + ks.T @ torch.cholesky_solve((y - c)[:, None], low)[:, 0]
    want_var = s - torch.linalg.solve_triangular(low, ks, upper=False).square().sum(dim=0)
    mean, var, obs = (t.cpu() for t in model.predict(xt))
    e_mean = ((mean - want_mean).abs().max() / s).item()
    e_var = ((var - want_var).abs().max() / s).item()
    e_obs = ((obs - (want_var + noise)).abs().max() / s).item()
    print(f"predict: mean {e_mean:.2e}, latent variance {e_var:.2e}, observation variance {e_obs:.2e} (relative to s)")
    assert e_mean <= 1e-11 and e_var <= 1e-10 and e_obs <= 1e-10


def test_hand_over_to_a_pls_step():
    """exact_gp_runner -> averaged kernel and noise -> PLSKernel -> OrthonormalBasis -> GaussianCost -> one particle update"""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.basis import OrthonormalBasis
    from projected_langevin_sampling_amd.costs import GaussianCost
    from projected_langevin_sampling_amd.link_functions import IdentityLinkFunction

    x, y = _training_data(600, 3, 24)
    models = pkg.exact_gp_runner(x, y, "rbf", subsample_size=200, seed=5, number_of_epochs=5, learning_rate=0.05,
                                 number_of_iterations=2, early_stopper_patience=10.0)
    assert len(models) == 2 and all(m.n == 200 for m in models)
    assert not torch.equal(models[0].x, models[1].x), "the two iterations drew the same subsample"
    kernel = pkg.construct_average_ard_kernel(models)
    noise = pkg.construct_average_gaussian_noise(models)
    assert isinstance(kernel, pkg.ARDKernel) and kernel.lengthscale.numel() == 3 and noise > 1e-4
    z = x[:24].clone()
    basis = OrthonormalBasis(pkg.PLSKernel(kernel, z), z, x, 1e-6, verbose=False)
    cost = GaussianCost(noise, y, IdentityLinkFunction())
    g = torch.Generator().manual_seed(25)
    u = torch.randn(basis.approximation_dimension, 16, generator=g, dtype=F64)
    update = pkg.PLS(basis, cost).calculate_particle_update(u.cuda(), 1e-3)
    assert update.shape == u.shape and torch.isfinite(update).all()
    assert len(pkg.exact_gp_runner(x[:50], y[:50], "matern", 200, 5, 2, 0.05, 3, 10.0)) == 1  # the subsample covers the data
