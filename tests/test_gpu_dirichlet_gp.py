"""GPU: Dirichlet exact-GP classification -- every class and output of pls_gp_mll_grad_classes against 50-digit
arithmetic, its anchors (a row is a one-class call; one class without fixed noise is pls_gp_mll_grad), a pivot reported
per class, the training loop against the same loop on the CPU, prediction, the class probabilities of
pls_softmax_normal_mean against the host restatement of the Philox stream, and the hand-over to a PLS step."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import dirichlet_gp_truth as T
import exact_gp_truth as E

pytestmark = pytest.mark.gpu

F64 = torch.float64


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


def padded(rows, pad):
    """(device (C, n + pad) matrix with NaN in the padding, its leading dimension)"""
    c, n = rows.shape
    buf = torch.full((c, n + pad), float("nan"), dtype=F64, device="cuda")
    buf[:, :n] = cu(rows)
    return buf, n + pad


def host_array(values):
    a = (ctypes.c_double * len(values))(*[float(v) for v in values])
    return a, ctypes.cast(a, ctypes.c_void_p)


def gp_classes(lib, kind, x, y, fixed, ls, s, sigma, mean, jitter=0.0, pad=3, fill=float("nan")):
    """pls_gp_mll_grad_classes through the C ABI with ldy = ldf = n + pad, a NaN-filled workspace and guards behind out and
    info: (out (C, 4 + d) on the CPU, info (C), status)"""
    L = _L()
    n, d = x.shape
    c = y.shape[0]
    xd, lsd = cu(x), cu(ls)
    yd, ldy = padded(y, pad)
    fd, ldf = padded(fixed, pad) if fixed is not None else (None, n)
    nbytes = lib.pls_gp_mll_classes_workspace_bytes(n, d, c)
    ws = torch.full((nbytes // 8,), fill, dtype=F64, device="cuda")
    out = torch.full((c * (4 + d) + 1,), float("nan"), dtype=F64, device="cuda")
    info = torch.full((c + 1,), -7, dtype=torch.int32, device="cuda")
    keep = [host_array(v.tolist()) for v in (s, sigma, mean)]
    rc = lib.pls_gp_mll_grad_classes(kind, xd.data_ptr(), n, d, c, lsd.data_ptr(), keep[0][1], keep[1][1], keep[2][1],
                                     fd.data_ptr() if fd is not None else None, ldf, yd.data_ptr(), ldy, float(jitter), out.data_ptr(),
                                     info.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr())
    host, flags = out.cpu(), info.cpu()
    assert torch.isnan(host[-1]), "the evaluation wrote past its C (4 + d) outputs"
    assert flags[-1].item() == -7, "the evaluation wrote past its C info words"
    assert torch.isnan(yd[:, n:]).all() and (fd is None or torch.isnan(fd[:, n:]).all())
    return host[:-1].reshape(c, 4 + d), flags[:-1].tolist(), rc


# ---- 1. every case against the 50 digits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_every_class_and_output_against_50_digits(lib, name):
    """Per class and output against the 50-digit truth, relative to the output's sum-of-magnitudes scale.  Bar, as for
    pls_gp_mll_grad: max(16 e_cpu, 64 eps), e_cpu the LAPACK helper's own error on the case (never the device's)."""
    kind, x, _, y, v, ls, s, sigma, mean = T.case_inputs(name)
    _, mag, e_cpu = T.cpu_case(name)
    hi, lo = T.truth(name)
    got, info, rc = gp_classes(lib, kind, x, y, v, ls, s, sigma, mean)
    assert rc == 0 and info == [0] * y.shape[0]
    err = E.relative_error(got.numpy(), hi, lo, mag)
    bar = np.maximum(16.0 * e_cpu, 64.0 * E.EPS)
    for c in range(y.shape[0]):
        print(f"{name} class {c}: max err/S {err[c].max():.2e}  max err/bar {np.max(err[c] / bar[c]):.3f}  (e_cpu max {e_cpu[c].max():.2e})"
              "  per output err/bar " + " ".join(f"{r:.3f}" for r in err[c] / bar[c]))
    again, _, _ = gp_classes(lib, kind, x, y, v, ls, s, sigma, mean, pad=0, fill=0.0)
    assert torch.equal(got, again), "two calls differ (or the result depends on the workspace's contents or on ldy / ldf)"
    assert np.all(err <= bar), (name, err / bar)


# ---- 2. anchors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rbf-n130-d3-c3", "matern32-n65-d1-c3", "matern32-n130-d3-c2"])
def test_a_row_is_a_one_class_call(lib, name):
    """row c of a C-class call == a one-class call with class c's parameters, bit for bit: strides, and anything a class
    leaves behind in the shared planes"""
    kind, x, _, y, v, ls, s, sigma, mean = T.case_inputs(name)
    got, info, rc = gp_classes(lib, kind, x, y, v, ls, s, sigma, mean)
    assert rc == 0 and not any(info)
    for c in range(y.shape[0]):
        one, info1, rc = gp_classes(lib, kind, x, y[c:c + 1], v[c:c + 1], ls[c:c + 1], s[c:c + 1], sigma[c:c + 1], mean[c:c + 1])
        assert rc == 0 and info1 == [0] and torch.equal(one[0], got[c]), (name, c)


@pytest.mark.parametrize("name", ["rbf-n130-d3", "matern32-n65-d8", "matern52-n2-d1"])
def test_one_class_without_fixed_noise_is_gp_mll_grad(lib, name):
    L = _L()
    kind, x, y, ls = E.case_inputs(name)
    n, d = x.shape
    one = lambda v: torch.tensor([v], dtype=F64)  # noqa: E731
    got, info, rc = gp_classes(lib, kind, x, y[None, :], None, ls[None, :], one(E.OUTPUTSCALE), one(E.NOISE), one(E.MEAN))
    assert rc == 0 and info == [0]
    xd, yd, lsd = cu(x), cu(y), cu(ls)
    nbytes = lib.pls_gp_mll_workspace_bytes(n, d)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    out = torch.zeros(4 + d, dtype=F64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    L.check(lib.pls_gp_mll_grad(kind, xd.data_ptr(), n, d, lsd.data_ptr(), E.OUTPUTSCALE, E.NOISE, E.MEAN, 0.0, yd.data_ptr(),
                                out.data_ptr(), flag.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "pls_gp_mll_grad")
    assert flag.item() == 0 and torch.equal(out.cpu(), got[0])


# ---- 3. a pivot is reported per class ----------------------------------------------------------------------------------------
def test_pivot_is_reported_for_its_class_alone(lib):
    """Two identical rows of x; class 1 has no fixed noise, sigma = 0 and outputscale 1: its second pivot is exactly 0
    (sqrt and the quotient are exact).  info = (0, 2, 0), PLS_OK, and classes 0 and 2 still meet the bar of the
    50-digit test (their truth is computed here, by the fixture's own script).  DirichletExactGP on the same data is
    fine (sigma >= 1e-4 and the fixed noise)."""
    import projected_langevin_sampling_amd as pkg

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_dirichlet_gp_truth as M

    g = torch.Generator().manual_seed(11)
    n, d = 66, 2
    x = torch.randn(n, d, generator=g, dtype=F64)
    x[1] = x[0]
    labels = torch.randint(0, 3, (n,), generator=g)
    y, v = pkg.dirichlet_targets(labels, 3)
    v[1] = 0.0
    ls = torch.tensor([[1.2, 0.9], [1.2, 1.2], [0.7, 1.6]], dtype=F64)
    s = torch.tensor([1.3, 1.0, 0.8], dtype=F64)
    sigma = torch.tensor([0.1, 0.0, 0.2], dtype=F64)
    mean = torch.tensor([0.2, 0.0, -0.3], dtype=F64)
    for kind in (E.RBF, E.MATERN32):
        got, info, rc = gp_classes(lib, kind, x, y, v, ls, s, sigma, mean)
        assert rc == 0 and info == [0, 2, 0], (kind, rc, info)
        for c in (0, 2):
            hi, lo = M.evaluate(kind, x.numpy(), y[c].numpy(), (v[c] + sigma[c]).numpy(), ls[c].numpy(), s[c].item(), mean[c].item())
            cpu, mag = E.mll_and_grad(kind, x, y[c], ls[c], s[c].item(), sigma[c].item(), mean[c].item(), v[c])
            bar = np.maximum(16.0 * E.relative_error(cpu, hi, lo, mag), 64.0 * E.EPS)
            err = E.relative_error(got[c].numpy(), hi, lo, mag)
            print(f"kind {kind} class {c} beside a failed class: max err/bar {np.max(err / bar):.3f}")
            assert np.all(err <= bar), (kind, c, err / bar)
    loss, grad = pkg.DirichletExactGP(x, labels, "rbf").loss_and_grad()
    assert np.isfinite(loss) and torch.isfinite(grad).all() and grad.shape == (3, 5)


# ---- 4. training ---------------------------------------------------------------------------------------------------------------
def _training_data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    score = torch.sin(1.5 * x[:, 0]) + 0.5 * x[:, -1] + 0.3 * torch.randn(n, generator=g, dtype=F64)
    return x, (score > 0).long()


@pytest.mark.parametrize("kernel", ["rbf", "matern32"])
def test_training_follows_the_cpu_loop(kernel):
    """train_exact_gp(likelihood="dirichlet") on the library against the same loop with the LAPACK helper.  The bar comes
    from the CPU loop alone, as in test_gpu_exact_gp.py: rerun with every gradient component perturbed by a relative 1e-12
    (alternating signs), 16 x the divergence of the losses and of the final raw parameters, floor 1e-11."""
    import projected_langevin_sampling_amd as pkg

    x, labels = _training_data(130, 2, 31)
    assert labels.sum().item() not in (0, 130)
    args = dict(seed=3, number_of_epochs=30, learning_rate=0.05, early_stopper_patience=10.0, likelihood="dirichlet")

    def perturbed(model):
        loss, grad = T.host_evaluate(model)
        sign = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(grad.numel())], dtype=F64).reshape(grad.shape)
        return loss, grad * (1.0 + 1e-12 * sign)

    cpu_model, cpu_losses = pkg.train_exact_gp(x, labels, kernel, evaluate=T.host_evaluate, **args)
    per_model, per_losses = pkg.train_exact_gp(x, labels, kernel, evaluate=perturbed, **args)
    gpu_model, gpu_losses = pkg.train_exact_gp(x, labels, kernel, **args)
    assert len(cpu_losses) == len(per_losses) == len(gpu_losses) == 30 and gpu_model.raw.shape == (2, 5)
    bar_loss = max(16.0 * np.abs(np.array(cpu_losses) - np.array(per_losses)).max(), 1e-11)
    bar_raw = max(16.0 * (cpu_model.raw_parameters() - per_model.raw_parameters()).abs().max().item(), 1e-11)
    d_loss = np.abs(np.array(cpu_losses) - np.array(gpu_losses)).max()
    d_raw = (cpu_model.raw_parameters() - gpu_model.raw_parameters()).abs().max().item()
    print(f"{kernel}: loss {cpu_losses[0]:.6f} -> {cpu_losses[-1]:.6f}; |gpu - cpu| losses {d_loss:.2e} (bar {bar_loss:.2e}), "
          f"raw {d_raw:.2e} (bar {bar_raw:.2e})")
    assert cpu_losses[-1] < cpu_losses[0] and gpu_losses[-1] < gpu_losses[0]
    assert d_loss <= bar_loss and d_raw <= bar_raw


# ---- 5. predict ------------------------------------------------------------------------------------------------------------------
def test_predict_against_the_helper():
    """Latent mean and variance per class against LAPACK at n = 130, t = 70, with the bars of test_gpu_exact_gp.py's
    test_predict_against_the_helper (1e-11 and 1e-10 relative to the outputscale, cond(K_y) <= 1e3)."""
    import projected_langevin_sampling_amd as pkg
    from matern_closed_form import matern_torch

    x, labels = _training_data(130, 2, 32)
    labels[::7] = 2
    g = torch.Generator().manual_seed(33)
    xt = torch.randn(70, 2, generator=g, dtype=F64)
    model = pkg.DirichletExactGP(x, labels, "matern52")
    model.set_raw_parameters(torch.tensor([[0.1, -1.5, 0.3, 0.2, 0.6], [-0.4, 0.5, 1.0, -0.3, 0.1], [0.0, -3.0, -0.5, 0.9, 0.4]], dtype=F64))
    mean, var = (t.cpu() for t in model.predict(xt))
    assert mean.shape == var.shape == (3, 70)
    for c in range(3):
        s, sigma, m, ls = model.outputscale[c].item(), model.noise[c].item(), model.mean_constant[c].item(), model.lengthscale[c]
        k = matern_torch(ls, s, 2.5)
        ky = k(x, x) + torch.diag(model.fixed_noise[c] + sigma)
        assert torch.linalg.cond(ky).item() <= 1e3
        low = torch.linalg.cholesky(ky)
        ks = k(x, xt)
        want_mean = m + ks.T @ torch.cholesky_solve((model.transformed_targets[c] - m)[:, None], low)[:, 0]
        want_var = s - torch.linalg.solve_triangular(low, ks, upper=False).square().sum(dim=0)
        e_mean = ((mean[c] - want_mean).abs().max() / s).item()
        e_var = ((var[c] - want_var).abs().max() / s).item()
        print(f"predict class {c}: mean {e_mean:.2e}, latent variance {e_var:.2e} (relative to s)")
        assert e_mean <= 1e-11 and e_var <= 1e-10
    proba = model.predict_proba(xt, number_of_samples=64, seed=5)
    want = T.proba(mean.numpy(), var.numpy(), 64, 5)
    assert proba.shape == (70, 3) and np.abs(proba.cpu().numpy() - want).max() <= T.proba_bar(mean.numpy(), var.numpy(), 64, 5)


# ---- 6. the class probabilities -------------------------------------------------------------------------------------------------
def softmax_mean(mu, var, samples, seed, first_point=0):
    """pls_softmax_normal_mean on (C, t) CPU inputs -> (t, C) numpy, with padded leading dimensions and NaN guards"""
    L = _L()
    lib = L.load()
    c, t = mu.shape
    md, ldm = padded(torch.as_tensor(mu, dtype=F64), 1)
    vd, ldv = padded(torch.as_tensor(var, dtype=F64), 2)
    out = torch.full((t, c + 1), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_softmax_normal_mean(md.data_ptr(), ldm, vd.data_ptr(), ldv, c, t, samples, seed, first_point, out.data_ptr(),
                                        c + 1, L.stream_ptr()), "pls_softmax_normal_mean")
    host = out.cpu()
    assert torch.isnan(host[:, c]).all(), "the kernel wrote into the padding of out"
    return host[:, :c].numpy()


def _latents(c, t, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(c, t, generator=g, dtype=F64)).numpy(), (4.0 * torch.rand(c, t, generator=g, dtype=F64)).numpy()


@pytest.mark.parametrize("samples", [1, 5, 13, 256, 4096])
@pytest.mark.parametrize("classes", [2, 3, 5])
@pytest.mark.parametrize("t", [1, 70])
def test_probabilities_against_the_restatement(t, classes, samples):
    """Bar, from the restatement alone (dirichlet_gp_truth.proba_bar): 16 x its change when every normal moves by
    8 eps max(1, |z|), plus eps x the additions on the longest path of the documented order."""
    seed, first = 1000 + samples, 3
    mu, var = _latents(classes, t, 100 * t + 10 * classes + samples % 7)
    want = T.proba(mu, var, samples, seed, first)
    bar = T.proba_bar(mu, var, samples, seed, first)
    got = softmax_mean(mu, var, samples, seed, first)
    err = np.abs(got - want).max()
    print(f"t={t} C={classes} S={samples}: max |device - restatement| {err:.2e}, bar {bar:.2e} ({err / bar:.3f})")
    assert np.array_equal(got, softmax_mean(mu, var, samples, seed, first)), "two calls differ"
    assert np.abs(got.sum(axis=1) - 1.0).max() <= bar
    assert err <= bar


def test_probability_edge_cases():
    mu, var = _latents(3, 6, 77)
    # sigma^2 = 0 (and below): softmax(mu) itself for every S.  Tolerance on entries <= 1: 8 eps for the exponentials'
    # roundings (1 ulp each, on the device and in numpy), the softmax's sum and its quotient, plus eps per addition of S copies
    want = T.softmax_rows(mu.T)
    for samples in (1, 13):
        got = softmax_mean(mu, np.where(np.arange(6) % 2 == 0, 0.0, -1.0) * np.ones((3, 1)), samples, 9)
        assert np.abs(got - want).max() <= E.EPS * (8 + T.longest_path_additions(samples))
    # a spread of means far beyond exp's range
    far = np.array([[800.0], [-800.0], [0.0]])
    got = softmax_mean(far, np.ones((3, 1)), 13, 9)
    assert np.all(np.isfinite(got)) and abs(got[0, 0] - 1.0) <= 8 * E.EPS and got[0, 1] == 0.0 and got[0, 2] == 0.0
    # first_point shifts the stream: points 3..5 of a t = 6 call are a t = 3 call that starts at 3
    whole = softmax_mean(mu, var, 37, 9)
    assert np.array_equal(whole[3:], softmax_mean(mu[:, 3:], var[:, 3:], 37, 9, first_point=3))
    assert not np.array_equal(whole[3:], softmax_mean(mu[:, 3:], var[:, 3:], 37, 9, first_point=0))


@pytest.mark.parametrize("classes", [12, 20, 64])
def test_probabilities_with_many_classes(classes):
    """the wider instantiations of the kernel (up to 16, 32 and 64 classes), same bar"""
    mu, var = _latents(classes, 3, classes)
    want, bar = T.proba(mu, var, 13, 21), T.proba_bar(mu, var, 13, 21)
    got = softmax_mean(mu, var, 13, 21)
    assert np.abs(got - want).max() <= bar and np.array_equal(got, softmax_mean(mu, var, 13, 21))


def test_quadrature_condition_through_the_device():
    """host test 6 through the kernel: within 4 standard errors of E sigma(g) by mpmath.quad, S = 4096, seed 7"""
    mu = np.array([p[0] for p in T.QUAD_PAIRS]).T.copy()
    var = np.array([p[1] for p in T.QUAD_PAIRS]).T.copy()
    got = softmax_mean(mu, var, T.QUAD_SAMPLES, T.QUAD_SEED)
    for i, (m, v) in enumerate(T.QUAD_PAIRS):
        want, se = T.quadrature(m, v)
        print(f"mu {m} var {v}: E sigma = {want:.6f}, device {got[i, 0]:.6f}, {abs(got[i, 0] - want) / se:.2f} standard errors")
        assert abs(got[i, 0] - want) <= 4.0 * se


# ---- 7. hand-over ------------------------------------------------------------------------------------------------------------------
def test_hand_over_to_a_pls_step():
    """exact_gp_runner(likelihood="dirichlet") -> class- and model-averaged kernel -> selector -> PLSKernel ->
    OrthonormalBasis -> BernoulliCost(sigmoid) -> one particle update"""
    import projected_langevin_sampling_amd as pkg
    from projected_langevin_sampling_amd.basis import OrthonormalBasis
    from projected_langevin_sampling_amd.costs import BernoulliCost
    from projected_langevin_sampling_amd.inducing_point_selectors import ConditionalVarianceInducingPointSelector
    from projected_langevin_sampling_amd.link_functions import SigmoidLinkFunction

    x, labels = _training_data(200, 2, 34)
    models = pkg.exact_gp_runner(x, labels, "rbf", subsample_size=120, seed=5, number_of_epochs=5, learning_rate=0.05,
                                 number_of_iterations=2, early_stopper_patience=10.0, likelihood="dirichlet")
    assert len(models) == 2 and all(type(m) is pkg.DirichletExactGP and m.n == 120 and m.number_of_classes == 2 for m in models)
    assert all(m.raw_parameters().abs().max().item() > 0 for m in models), "nothing was learned"
    kernel = pkg.construct_average_ard_kernel(models)
    assert isinstance(kernel, pkg.ARDKernel) and kernel.lengthscale.numel() == 2
    z, picked = ConditionalVarianceInducingPointSelector()(x, 14, kernel)
    assert z.shape == (14, 2) and len(set(picked.tolist())) == 14
    basis = OrthonormalBasis(pkg.PLSKernel(kernel, z), z, x, 1e-6, verbose=False)
    cost = BernoulliCost(labels.double(), SigmoidLinkFunction())
    g = torch.Generator().manual_seed(35)
    u = torch.randn(basis.approximation_dimension, 16, generator=g, dtype=F64)
    update = pkg.PLS(basis, cost).calculate_particle_update(u.cuda(), 1e-3)
    assert update.shape == u.shape and torch.isfinite(update).all()
