"""CPU: the host side of Dirichlet exact-GP classification -- the label transform, the LAPACK yardstick against 50-digit
arithmetic, the softplus chain rule per class against autograd, the training loop (stop rule, loss summed over classes,
Adam per class), the averaging order, the runner's class count and subsample quirk, the argument checks of the two new
C-ABI entry points (they run before any HIP call), and the host restatement of the class probabilities against quadrature."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dirichlet_gp_truth as T
import exact_gp_truth as E
import projected_langevin_sampling_amd as pkg
from projected_langevin_sampling_amd.gaussian_process import NOISE_LOWER_BOUND

L = pkg._lib
F64 = torch.float64
softplus = torch.nn.functional.softplus


# ---- 1. the transform ----------------------------------------------------------------------------------------------------
def test_transform_literals_rounding_class_count_and_range():
    labels = torch.tensor([0, 1, 1, 0, 1])
    y64, v64 = pkg.dirichlet_targets(labels, target_dtype=torch.float64)
    assert y64.shape == v64.shape == (2, 5) and y64.dtype == v64.dtype == F64
    for c in range(2):
        for i, lab in enumerate(labels.tolist()):
            v, y = T.LITERALS[1.01 if lab == c else 0.01]
            assert abs(v64[c, i].item() - v) <= 2 * E.EPS * abs(v) and abs(y64[c, i].item() - y) <= 2 * E.EPS * abs(y)
    want_y, want_v = T.transform(labels.tolist(), 2)
    assert (y64 - want_y).abs().max().item() <= 4 * E.EPS * 7 and (v64 - want_v).abs().max().item() <= 4 * E.EPS * 5
    # the default rounds both to float32 (gpytorch's dtype argument) and promotes them to float64
    y32, v32 = pkg.dirichlet_targets(labels)
    assert y32.dtype == v32.dtype == F64
    for c in range(2):
        for i, lab in enumerate(labels.tolist()):
            v, y = T.LITERALS[1.01 if lab == c else 0.01]
            assert v32[c, i].item() == float(np.float32(v)) and y32[c, i].item() == float(np.float32(y))
    assert not torch.equal(y32, y64)
    model = pkg.DirichletExactGP(torch.arange(5.0), labels)
    assert torch.equal(model.transformed_targets, y32) and torch.equal(model.fixed_noise, v32) and model.number_of_classes == 2
    assert torch.equal(pkg.DirichletExactGP(torch.arange(5.0), labels, target_dtype=torch.float64).transformed_targets, y64)
    # more classes than the labels show: the absent classes are all "not observed"
    y4, v4 = pkg.dirichlet_targets(labels, number_of_classes=4)
    assert y4.shape == (4, 5) and torch.equal(y4[:2], y32) and torch.equal(v4[:2], v32)
    assert (y4[2:] == float(np.float32(T.LITERALS[0.01][1]))).all() and (v4[2:] == float(np.float32(T.LITERALS[0.01][0]))).all()
    assert pkg.DirichletExactGP(torch.arange(5.0), labels, number_of_classes=4).raw.shape == (4, 4)
    for bad in (dict(labels=torch.tensor([0, 2]), number_of_classes=2), dict(labels=torch.tensor([-1, 0])),
                dict(labels=torch.tensor([0.5, 1.0])), dict(labels=torch.tensor([0, 1]), number_of_classes=0)):
        with pytest.raises(ValueError):
            pkg.dirichlet_targets(**bad)
    with pytest.raises(ValueError):
        pkg.DirichletExactGP(torch.arange(2.0), torch.tensor([0, 3]), number_of_classes=3)


def test_the_case_table_is_the_issue_s():
    got = {(k, n, d, c) for k, n, d, c, _ in T.CASES.values()}
    assert got == {(k, n, d, c) for k in (E.RBF, E.MATERN32) for n in (2, 65, 130) for d in (1, 3) for c in (2, 3)}
    for name in T.CASES:
        _, _, labels, y, v, ls, s, sigma, mean = T.case_inputs(name)
        c = T.CASES[name][3]
        assert labels.dtype == torch.int64 and 0 <= labels.min() and labels.max() < c
        for per_class in (s, sigma, mean, ls[:, 0]):
            assert len(set(per_class.tolist())) == c, "class parameters must be distinct"
        assert torch.equal(y, y.float().double()) and torch.equal(v, v.float().double())


@pytest.mark.parametrize("name", list(T.CASES))
def test_lapack_yardstick_against_50_digits(name):
    """e_cpu per class and output, relative to the output's sum of magnitudes.  Bound as in test_exact_gp_host.py: the
    forward error of a backward-stable solve / inverse, cond(K_y) eps; the diagonal here is at least 0.05 + 0.688 under an
    outputscale below 1.8, so cond <= 2e3 holds with room.  The GPU tests take their bar from the measured e_cpu."""
    kind, x, _, y, v, ls, s, sigma, mean = T.case_inputs(name)
    _, mag, e_cpu = T.cpu_case(name)
    for c in range(y.shape[0]):
        ky = s[c] * E.kappa(kind, x, ls[c]) + torch.diag(v[c] + sigma[c])
        assert torch.linalg.cond(ky).item() <= 2e3
    print(f"{name}: e_cpu max {e_cpu.max():.1e}")
    assert e_cpu.shape == (y.shape[0], 4 + x.shape[1]) and np.all(e_cpu <= 2e3 * E.EPS), e_cpu


# ---- 2. the gradient against autograd -------------------------------------------------------------------------------------
def _autograd_loss(kind, x, targets, fixed, raw):
    """-sum_c mll_c / n as a differentiable function of raw (C, 3 + nls): torch autograd through LAPACK"""
    n, d = x.shape
    total = 0.0
    off = ~torch.eye(n, dtype=torch.bool)
    for c in range(raw.shape[0]):
        mean, sigma, s = raw[c, 0], NOISE_LOWER_BOUND + softplus(raw[c, 1]), softplus(raw[c, 2])
        ls = softplus(raw[c, 3:]).expand(d)
        e2 = ((x[:, None, :] - x[None, :, :]) / ls).square().sum(-1)
        if kind == E.RBF:
            kap = torch.exp(-0.5 * e2)
        else:  # Matern-3/2; sqrt has no derivative at 0: the diagonal is taken out before it
            t = torch.sqrt(3.0 * torch.where(off, e2, torch.ones_like(e2)))
            kap = torch.where(off, (1.0 + t) * torch.exp(-t), torch.ones_like(e2))
        low = torch.linalg.cholesky(s * kap + torch.diag(fixed[c] + sigma))
        r = targets[c] - mean
        alpha = torch.cholesky_solve(r[:, None], low)[:, 0]
        total = total + (-0.5 * r @ alpha - torch.log(low.diagonal()).sum() - 0.5 * n * math.log(2.0 * math.pi))
    return -total / n


@pytest.mark.parametrize("kernel,kind", [("rbf", E.RBF), ("matern32", E.MATERN32)])
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
@pytest.mark.parametrize("classes", [2, 3])
def test_chain_rule_against_autograd(kernel, kind, ard, classes):
    g = torch.Generator().manual_seed(60 + kind + 2 * ard + 10 * classes)
    n, d = 30, 3
    x = torch.randn(n, d, generator=g, dtype=F64)
    labels = torch.randint(0, classes, (n,), generator=g)
    model = pkg.DirichletExactGP(x, labels, kernel, ard=ard, number_of_classes=classes)
    nls = d if ard else 1
    assert model.raw.shape == (classes, 3 + nls) and not model.raw_parameters().any()  # every raw value starts at 0
    assert torch.equal(model.noise, torch.full((classes,), 1e-4 + math.log(2.0), dtype=F64))
    raw = torch.randn(classes, 3 + nls, generator=g, dtype=F64) * 0.5
    model.set_raw_parameters(raw)
    loss, grad = T.host_evaluate(model)
    leaf = raw.clone().requires_grad_(True)
    want = _autograd_loss(kind, x, model.transformed_targets, model.fixed_noise, leaf)
    want.backward()
    assert grad.shape == raw.shape
    assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
    assert (grad - leaf.grad).abs().max().item() <= 1e-11 * leaf.grad.abs().max().item()
    kernels = model.kernels
    assert len(kernels) == classes
    for c, k in enumerate(kernels):
        assert type(k) is (pkg.ARDKernel if kind == E.RBF else pkg.MaternKernel) and k.kind == kind
        assert torch.equal(k.lengthscale, softplus(raw[c, 3:]).expand(d)) and k.outputscale == softplus(raw[c, 2]).item()
    assert torch.equal(model.mean_constant, raw[:, 0]) and torch.equal(model.noise, 1e-4 + softplus(raw[:, 1]))


# ---- 3. the training loop --------------------------------------------------------------------------------------------------
def _data(n=40, d=2, classes=3, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.randint(0, classes, (n,), generator=g)


def test_training_loop_sums_the_classes_and_checks_the_stop_rule_first():
    x, labels = _data()
    args = dict(seed=1, number_of_epochs=12, learning_rate=0.05, early_stopper_patience=10.0, likelihood="dirichlet")
    model, losses = pkg.train_exact_gp(x, labels, "rbf", evaluate=T.host_evaluate, **args)
    assert type(model) is pkg.DirichletExactGP and model.raw.shape == (3, 5)
    assert len(losses) == 12 and all(b < a for a, b in zip(losses, losses[1:])), losses
    # the first loss is the SUM over the classes of -mll_c / n at the starting point
    start = pkg.DirichletExactGP(x, labels, "rbf")
    out, _ = T.mll_and_grad(start.kind, x, start.transformed_targets, start.fixed_noise, start.lengthscale, start.outputscale,
                            start.noise, start.mean_constant)
    assert losses[0] == -float(torch.from_numpy(out[:, 0]).sum()) / 40
    assert abs(losses[0] + math.fsum(out[:, 0].tolist()) / 40) <= 4 * E.EPS * abs(losses[0])
    calls, seen = [], []

    def nan_on_fourth(m):
        calls.append(1)
        seen.append(m.raw_parameters())
        loss, grad = T.host_evaluate(m)
        return (float("nan") if len(calls) == 4 else loss), grad

    stopped, kept = pkg.train_exact_gp(x, labels, "rbf", evaluate=nan_on_fourth, **args)
    assert len(calls) == 4 and kept == losses[:3]
    assert torch.equal(stopped.raw_parameters(), seen[3]) and not torch.equal(seen[3], seen[2])  # no step after the stop
    with pytest.raises(ValueError):
        pkg.train_exact_gp(x, labels, "rbf", 1, 1, 0.05, 10.0, likelihood="bernoulli")
    # the default is the Gaussian model, as before
    assert type(pkg.train_exact_gp(x, labels.double(), "rbf", 1, 0, 0.05, 10.0)[0]) is pkg.ExactGP


def test_adam_on_the_class_matrix_is_adam_per_class():
    x, labels = _data()
    model, _ = pkg.train_exact_gp(x, labels, "matern32", 2, 8, 0.05, 10.0, evaluate=T.host_evaluate, likelihood="dirichlet")
    twin = pkg.DirichletExactGP(x, labels, "matern32")
    rows = [torch.nn.Parameter(torch.zeros(5, dtype=F64)) for _ in range(3)]
    optimizers = [torch.optim.Adam([r], lr=0.05) for r in rows]
    for _ in range(8):
        twin.set_raw_parameters(torch.stack([r.detach() for r in rows]))
        _, grad = T.host_evaluate(twin)
        for c, (r, opt) in enumerate(zip(rows, optimizers)):
            opt.zero_grad()
            r.grad = grad[c].clone()
            opt.step()
    assert torch.equal(model.raw_parameters(), torch.stack([r.detach() for r in rows]))


# ---- 4. averaging and the runner -------------------------------------------------------------------------------------------
def test_classes_are_averaged_first_then_models_then_softplus():
    x, labels = _data(10, 2, 2)
    a = pkg.DirichletExactGP(x, labels, "matern32").set_raw_parameters(
        torch.tensor([[0.3, -2.0, 1.0, -1.0, 2.0], [0.5, 0.0, 3.0, 1.0, 0.0]], dtype=F64))
    b3 = pkg.DirichletExactGP(x, torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2, 0]), "matern32").set_raw_parameters(
        torch.tensor([[0.1, 1.0, -3.0, 3.0, -1.0], [0.0, 0.0, 0.0, 0.0, 2.0], [0.0, 0.0, 6.0, 0.0, -4.0]], dtype=F64))
    # per model over its classes: a -> (2, 0, 1), b3 -> (1, 1, -1); then the models: (1.5, 0.5, 0); then softplus
    k = pkg.construct_average_ard_kernel([a, b3])
    assert type(k) is pkg.MaternKernel and k.nu == 1.5
    assert torch.equal(k.lengthscale, softplus(torch.tensor([0.5, 0.0], dtype=F64)))
    assert k.outputscale == softplus(torch.tensor(1.5, dtype=F64)).item()
    # (all five class rows at once would give an outputscale raw of 7/5, the average of the natural values something else again)
    assert abs(k.outputscale - softplus(torch.tensor(1.4, dtype=F64)).item()) > 0.05
    own = a.kernel
    assert torch.equal(own.lengthscale, softplus(torch.tensor([0.0, 1.0], dtype=F64))) and own.outputscale == softplus(torch.tensor(2.0, dtype=F64)).item()
    natural = torch.stack([kk.lengthscale for kk in a.kernels]).mean(dim=0)
    assert (own.lengthscale - natural).abs().max().item() > 0.05
    assert type(pkg.construct_average_ard_kernel([pkg.DirichletExactGP(x, labels, "rbf", ard=False)])) is pkg.ARDKernel


def test_runner_class_count_and_the_subsample_quirk():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(60, 2, generator=g, dtype=F64)
    x[50:] += 100.0  # class 2 lives far away: no 20-point neighbourhood of the near cloud holds it
    labels = torch.cat([torch.randint(0, 2, (50,), generator=g), torch.full((10,), 2)])
    args = dict(subsample_size=20, seed=0, number_of_epochs=0, learning_rate=0.05, number_of_iterations=4,
                early_stopper_patience=10.0, likelihood="dirichlet")  # (0 epochs: the models are built, nothing is evaluated)
    models = pkg.exact_gp_runner(x, labels, "rbf", **args)
    assert len(models) == 4 and all(type(m) is pkg.DirichletExactGP and m.n == 20 for m in models)
    assert any(int(m.labels.max()) < 2 for m in models), "no subsample lacks a class: the test shows nothing"
    assert all(m.number_of_classes == 3 and m.raw.shape == (3, 5) and m.fixed_noise.shape == (3, 20) for m in models)
    assert all(pkg.exact_gp_runner(x, labels, "rbf", number_of_classes=5, **args)[i].number_of_classes == 5 for i in range(4))
    # the fixed noise rows follow the subsample (the default) ...
    m = models[0]
    assert torch.equal(m.fixed_noise, pkg.dirichlet_targets(m.labels, 3)[1])
    # ... or are dropped as in the reference, but only when the subsample is smaller than the data
    quirk = pkg.exact_gp_runner(x, labels, "rbf", subsample_fixed_noise=False, **args)
    assert all(q.fixed_noise is None and torch.equal(q.transformed_targets, mm.transformed_targets) for q, mm in zip(quirk, models))
    whole = pkg.exact_gp_runner(x, labels, "rbf", **{**args, "subsample_size": 60, "subsample_fixed_noise": False})
    assert len(whole) == 1 and whole[0].n == 60 and whole[0].fixed_noise is not None and whole[0].fixed_noise.shape == (3, 60)
    with pytest.raises(ValueError):
        pkg.exact_gp_runner(x, labels, "rbf", **{**args, "likelihood": "poisson"})


# ---- 5. argument checks -----------------------------------------------------------------------------------------------------
def test_cabi_argument_checks_run_before_any_hip_call():
    lib = L.load()
    p = 16  # any non-NULL address: no device pointer is dereferenced before the checks pass
    host = (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    negative = (ctypes.c_double * 3)(0.5, -1e-9, 0.5)
    nan = (ctypes.c_double * 3)(0.5, 0.5, float("nan"))
    hp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def classes(kind=0, x=p, n=4, d=2, c=3, ls=p, s=hp(host), noise=hp(host), mean=hp(host), fixed=p, ldf=4, y=p, ldy=4, jitter=0.0,
                out=p, info=p, ws=p, nbytes=1 << 20):
        return (lib.pls_gp_mll_grad_classes(kind, x, n, d, c, ls, s, noise, mean, fixed, ldf, y, ldy, jitter, out, info, ws, nbytes, None),
                lib.pls_last_error())

    assert classes(kind=5)[0] == 1 and b"unknown kernel kind 5" in classes(kind=5)[1]
    assert classes(kind=L.KERNEL_LINEAR)[0] == 1 and b"linear kernel" in classes(kind=L.KERNEL_LINEAR)[1]
    for bad in (dict(n=0), dict(n=-3), dict(d=0), dict(c=0), dict(c=-1)):
        assert classes(**bad)[0] == 1 and b"bad sizes" in classes(**bad)[1], bad
    assert classes(d=65)[0] == 1 and b"> 64 is not supported" in classes(d=65)[1]
    for name in ("x", "ls", "s", "noise", "mean", "y", "out", "info"):
        assert classes(**{name: None})[0] == 1 and b"NULL pointer" in classes(**{name: None})[1], name
    assert classes(ldy=3)[0] == 1 and b"ldy < n" in classes(ldy=3)[1]
    assert classes(ldf=3)[0] == 1 and b"ldf < n" in classes(ldf=3)[1]
    assert classes(jitter=-1.0)[0] == 1 and b"jitter" in classes(jitter=-1.0)[1]
    assert classes(ws=None)[0] == 1 and b"NULL workspace" in classes(ws=None)[1]
    rc, msg = classes(nbytes=8)
    assert rc == 3 and b"workspace of 8 bytes" in msg, msg
    assert classes(ws=24)[0] == 1 and b"16-byte aligned" in classes(ws=24)[1]
    assert classes(noise=hp(negative))[0] == 1 and b"noise must be >= 0 (class 1)" in classes(noise=hp(negative))[1]
    assert classes(noise=hp(nan))[0] == 1 and b"(class 2)" in classes(noise=hp(nan))[1]
    # the classes share the planes of one evaluation
    assert lib.pls_gp_mll_classes_workspace_bytes(5, 3, 4) == lib.pls_gp_mll_workspace_bytes(5, 3) == 8 * (7 * 5 * 6 + 2 * 6 + 4 + 4)
    assert lib.pls_gp_mll_classes_workspace_bytes(5, 3, 0) == 0 and lib.pls_gp_mll_classes_workspace_bytes(0, 3, 2) == 0

    def proba(mu=p, ldmu=7, var=p, ldvar=7, c=3, t=7, samples=5, out=p, ldo=3):
        return lib.pls_softmax_normal_mean(mu, ldmu, var, ldvar, c, t, samples, 1, 0, out, ldo, None), lib.pls_last_error()

    for bad in (dict(c=0), dict(t=0), dict(samples=0), dict(t=-2), dict(samples=-1)):
        assert proba(**bad)[0] == 1 and b"bad sizes" in proba(**bad)[1], bad
    assert proba(c=65, ldo=65)[0] == 1 and b"> 64 are not supported" in proba(c=65, ldo=65)[1]
    for name in ("mu", "var", "out"):
        assert proba(**{name: None})[0] == 1 and b"NULL pointer" in proba(**{name: None})[1], name
    assert proba(ldmu=6)[0] == 1 and proba(ldvar=6)[0] == 1 and b"< t" in proba(ldvar=6)[1]
    assert proba(ldo=2)[0] == 1 and b"ldo < classes" in proba(ldo=2)[1]


# ---- 6. the host restatement of the probabilities -----------------------------------------------------------------------------
def test_restatement_against_quadrature():
    """Two classes: softmax_0 = sigma(f0 - f1), f0 - f1 ~ N(mu0 - mu1, var0 + var1).  The restatement's mean of S = 4096
    draws must lie within 4 standard errors of E sigma(g), both by mpmath.quad -- a condition on the stream, not a
    measurement of the code.  On these five pairs the restatement is at 0.38, 0.54, 0.93, 1.04 and 1.76 standard errors."""
    assert ((-2.0, 1.0), (9.0, 16.0)) in T.QUAD_PAIRS and len(T.QUAD_PAIRS) == 5
    worst = 0.0
    for i, (mu, var) in enumerate(T.QUAD_PAIRS):
        want, se = T.quadrature(mu, var)
        got = T.proba_point(mu, var, T.QUAD_SAMPLES, T.QUAD_SEED, i)
        z = abs(got[0] - want) / se
        worst = max(worst, z)
        print(f"mu {mu} var {var}: E sigma = {want:.6f}, restatement {got[0]:.6f}, {z:.2f} standard errors ({se:.2e})")
        assert abs(got.sum() - 1.0) <= 8 * E.EPS and z <= 4.0
    print(f"worst {worst:.2f} standard errors")
    # sigma^2 = 0: the softmax of the means itself; a huge spread of means stays finite
    assert np.array_equal(T.proba_point((1.0, -2.0, 0.5), (0.0, 0.0, 0.0), 5, 3, 0), T.proba_point((1.0, -2.0, 0.5), (-1.0, 0.0, 0.0), 1, 3, 0))
    assert np.all(np.isfinite(T.proba_point((800.0, -800.0, 0.0), (1.0, 1.0, 1.0), 13, 3, 0)))
