"""CPU: the host side of the periodic base kernel -- the closed-form yardstick against 50-digit arithmetic (a per-pair table
and three whole evaluations), the kernel class and the gpytorch-shaped objects as_base_kernel reads, the raw parameter
layout of ExactGP / DirichletExactGP with the raw period lengths behind the raw lengthscales, chain_rule against central
differences, the averaging constructor, and the C ABI's argument checks and kind-aware workspace queries (they run before
any HIP call)."""
import numpy as np
import pytest
import torch

import periodic_truth as T
import projected_langevin_sampling_amd as pkg
from periodic_closed_form import LN2, periodic_factors_numpy, periodic_numpy, periodic_torch, sensitivity
from projected_langevin_sampling_amd.kernel import ARDKernel, PeriodicKernel, RQKernel, as_base_kernel

L = pkg._lib
F64 = torch.float64
sp = torch.nn.functional.softplus


# ---- the yardstick -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(T.PAIR_PERIODS)), ids=[f"p={p:g}" for p in T.PAIR_PERIODS])
def test_numpy_helper_against_50_digits(k):
    """kappa, fl and fp of periodic_factors_numpy per pair of the fixture's table.  Bars from the formulas.  The reduced angle
    theta = pi r carries dth = (pi |e| / 2 + pi / 2) eps absolute: the rounding of e = delta / p, |e| eps / 2 (absent for the
    power-of-two periods, whose quotient is exact), times pi, and the rounding of the product pi r with that of the sine
    and cosine near pi / 2 (numpy's cos(pi r) does not know that r = 1/2 is a zero), pi / 2 eps together.  With q = fl the
    negated exponent and |d sin^2 / d theta| = |sin 2 theta| <= 1, |d sin 2 theta / d theta| <= 2:
        kappa: (3 q + 8) eps kappa + kappa (2 / lambda) dth
        fl:    8 fl eps + (2 / lambda) dth
        fp:    8 |fp| eps + (2 / lambda) pi |e| (2 dth + eps / 2)          (the last: e itself, in front)
    At e = 2^52 and 1e15 + 0.5 with p = 0.7 the bars are of order 1 and e^2: delta / p is not representable there and no
    float64 evaluation can know the phase; with p = 1 and 2^-3 only the pi / 2 eps of the angle remain."""
    p, lam = T.PAIR_PERIODS[k], T.PAIR_LENGTHSCALE
    hi, lo = T.pair_truth()
    delta = T.pair_deltas()[k]
    kap, fl, fp, e = periodic_factors_numpy(delta[:, None], [lam], [p])
    fl, fp, e = fl[:, 0], fp[:, 0], e[:, 0]
    inexact = 0.0 if p != 0.7 else 1.0  # (p = 1 and 2^-3: the quotient and its reduction are exact)
    dth = (np.pi * np.abs(e) * 0.5 * inexact + np.pi / 2.0) * T.EPS
    bars = {"kappa": (3.0 * fl + 8.0) * T.EPS * hi[k, 0] + hi[k, 0] * (2.0 / lam) * dth,
            "fl": 8.0 * hi[k, 1] * T.EPS + (2.0 / lam) * dth,
            "fp": 8.0 * np.abs(hi[k, 2]) * T.EPS + (2.0 / lam) * np.pi * np.abs(e) * (2.0 * dth + 0.5 * T.EPS * inexact)}
    for row, (name, got) in enumerate((("kappa", kap), ("fl", fl), ("fp", fp))):
        err = np.abs((got - hi[k, row]) - lo[k, row])
        bar = bars[name] + 1e-300  # (the floor: entries that are subnormal or 0)
        print(f"p={p:g} {name}: max err/bar {np.max(err / bar):.3f}")
        assert np.all(err <= bar), (name, err / bar)
    assert kap[0] == 1.0 and fl[0] == 0.0 and fp[0] == 0.0, "distance 0: kappa = 1 and both factors 0 exactly"
    if p != 0.7:
        whole = np.isin(T.PAIR_E, [1.0, 2.0**52])
        assert np.all(kap[whole] == 1.0) and np.all(fl[whole] == 0.0), "a whole number of periods apart: kappa = 1 exactly"


def test_closed_forms_agree_and_hold_the_diagonal():
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(7, 3, generator=g, dtype=F64), torch.randn(9, 3, generator=g, dtype=F64)
    ls, period = 0.5 + torch.rand(3, generator=g, dtype=F64), 0.5 + 2.5 * torch.rand(3, generator=g, dtype=F64)
    a, b = periodic_torch(ls, 2.5, period)(x1, x2).numpy(), periodic_numpy(ls.numpy(), 2.5, period.numpy())(x1.numpy(), x2.numpy())
    assert np.abs(a - b).max() <= 16 * T.EPS * 2.5  # (the exponent is O(1) here: a few eps from each sine library)
    assert np.all(periodic_torch(ls, 2.5, period)(x1, x1).diagonal().numpy() == 2.5)
    assert np.all(np.diag(periodic_numpy(ls.numpy(), 2.5, period.numpy())(x1.numpy(), x1.numpy())) == 2.5)
    far = torch.full((1, 3), float("inf"), dtype=F64)
    assert torch.isnan(periodic_torch(ls, 1.0, period)(far, -far)).all(), "no limit at infinity: NaN"
    assert np.isnan(periodic_numpy(ls.numpy(), 1.0, period.numpy())(far.numpy(), -far.numpy())).all()


@pytest.mark.parametrize("name", list(T.CASES))
def test_lapack_helper_is_a_legitimate_yardstick(name):
    """periodic_truth.mll_and_grad against the 50-digit truth, per output relative to its sum-of-magnitudes scale S.  The GPU
    bar of test_gpu_periodic is max(16 e_cpu, 64 eps); the helper's own error must be at most 1/16 of it.  That alone holds by
    construction, so the helper is also held to what a backward-stable Cholesky evaluation can show: n cond(K_y) eps
    relative to S (Higham, Accuracy and Stability, thm. 10.4 with the growth factor n)."""
    x, y, ls, period = T.case_inputs(name)
    n, d = x.shape
    out, mag, e_cpu = T.cpu_case(name)
    assert out.shape == mag.shape == (4 + 2 * d,) and np.all(mag > 0)
    gpu_bar = np.maximum(16.0 * e_cpu, 64.0 * T.EPS)
    ky = T.OUTPUTSCALE * T.kappa(x, ls, period) + T.NOISE * torch.eye(n, dtype=F64)
    cond = torch.linalg.cond(ky).item()
    print(f"{name}: e_cpu max {e_cpu.max():.2e} = {e_cpu.max() / T.EPS:.1f} eps, cond(K_y) {cond:.1e}, per output " +
          " ".join(f"{v / T.EPS:.1f}" for v in e_cpu))
    assert np.all(e_cpu <= gpu_bar / 16.0) and np.all(e_cpu <= n * cond * T.EPS)
    kap = T.kappa(x, ls, period)
    assert (kap > 1e-3).double().mean().item() >= 0.5, "test construction: most entries must be of the size of s"


# ---- kernel objects ------------------------------------------------------------------------------------------------------
def _scale_stub(lengthscale, outputscale, **inner_attributes):
    inner = type("Inner", (), {"lengthscale": lengthscale, **inner_attributes})()
    return type("ScaleStub", (), {"base_kernel": inner, "outputscale": outputscale})()


def test_periodic_kernel_class_and_validation():
    k = PeriodicKernel([0.5, 2.0, 1.25], 3.0, period_length=[1.0, 0.7, 2.5])
    assert k.kind == L.KERNEL_PERIODIC == T.PERIODIC == 8 and k.outputscale == 3.0
    assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.period_length.tolist() == [1.0, 0.7, 2.5]
    assert k._lengthscale_host(3).tolist() == [0.5, 2.0, 1.25, 1.0, 0.7, 2.5], "the library reads the periods behind the lengthscales"
    shared = PeriodicKernel([0.75], 1.5, period_length=2.0)
    assert shared._lengthscale_host(4).tolist() == [0.75] * 4 + [2.0] * 4
    assert PeriodicKernel([1.0, 2.0], period_length=0.5)._lengthscale_host(2).tolist() == [1.0, 2.0, 0.5, 0.5]
    assert PeriodicKernel([1.0]).period_length.tolist() == [1.0] and PeriodicKernel([1.0]).outputscale == 1.0
    assert pkg.PeriodicKernel is PeriodicKernel and "PeriodicKernel" in pkg.__all__
    from projected_langevin_sampling_amd.kernel import _StationaryKernel
    assert isinstance(k, _StationaryKernel)
    for bad in (0.0, -1.0, [1.0, 0.0], float("nan")):
        with pytest.raises(ValueError, match="period length"):
            PeriodicKernel([1.0, 1.0], 1.0, period_length=bad)
    with pytest.raises(ValueError, match="lengthscale"):
        PeriodicKernel([1.0, -1.0], 1.0)
    with pytest.raises(AssertionError, match="has 3 entries, data has 2 dims"):
        k._lengthscale_host(2)


def test_as_base_kernel_reads_a_scale_periodic_kernel():
    k = as_base_kernel(_scale_stub(torch.tensor([[0.5, 2.0, 1.25]]), torch.tensor(3.0), period_length=torch.tensor([[1.0, 0.75, 2.5]])))
    assert type(k) is PeriodicKernel and k.outputscale == 3.0
    assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.period_length.tolist() == [1.0, 0.75, 2.5]
    k = as_base_kernel(_scale_stub(torch.tensor([[0.75]]), 1.5, period_length=torch.tensor([[2.0]])))  # shared values
    assert type(k) is PeriodicKernel and k._lengthscale_host(2).tolist() == [0.75, 0.75, 2.0, 2.0]
    assert as_base_kernel(k) is k
    assert type(as_base_kernel(_scale_stub(torch.tensor([[1.0]]), 1.0, alpha=2.0))) is RQKernel
    assert type(as_base_kernel(_scale_stub(torch.tensor([[1.0]]), 1.0))) is ARDKernel


# ---- the raw layout ------------------------------------------------------------------------------------------------------
def _data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.sin(x.sum(dim=1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)


def test_exact_gp_raw_layout_and_start_values():
    x, y = _data(12, 3, 1)
    model = pkg.ExactGP(x, y, kernel=PeriodicKernel)
    assert model.kind == L.KERNEL_PERIODIC and model.kernel_name == "periodic" and model.raw.shape == (9,)  # 3 + 2 nls
    assert torch.equal(model.raw.detach(), torch.zeros(9, dtype=F64))
    assert model.period_length.shape == (3,) and torch.allclose(model.period_length, torch.full((3,), LN2, dtype=F64), rtol=1e-15)
    assert torch.allclose(model.lengthscale, torch.full((3,), LN2, dtype=F64), rtol=1e-15)
    assert not hasattr(model, "alpha") and not hasattr(pkg.ExactGP(x, y, kernel="rbf"), "period_length")
    shared = pkg.ExactGP(x, y, kernel=PeriodicKernel, ard=False)
    assert shared.raw.shape == (5,) and shared.period_length.shape == (3,) and shared._library_lengthscale().shape == (1, 6)
    start = PeriodicKernel([0.5, 2.0, 1.25], 1.7, period_length=[1.0, 0.7, 2.5])
    model = pkg.ExactGP(x, y, kernel=start)
    assert model.kind == L.KERNEL_PERIODIC and model.ard and model.raw.shape == (9,)
    assert torch.allclose(model.lengthscale, start.lengthscale, rtol=1e-14)
    assert torch.allclose(model.period_length, start.period_length, rtol=1e-14) and model.outputscale == pytest.approx(1.7, rel=1e-14)
    fitted = model.kernel
    assert type(fitted) is PeriodicKernel and fitted.outputscale == model.outputscale
    assert torch.equal(fitted.lengthscale, model.lengthscale) and torch.equal(fitted.period_length, model.period_length)
    one = pkg.ExactGP(x, y, kernel=PeriodicKernel([0.8], 1.1, period_length=[1.3]))
    assert not one.ard and one.raw.shape == (5,)
    assert torch.allclose(one.period_length, torch.full((3,), 1.3, dtype=F64), rtol=1e-14)
    mixed = pkg.ExactGP(x, y, kernel=PeriodicKernel([0.8], 1.1, period_length=[1.0, 0.7, 2.5]))  # per-dimension periods: ard
    assert mixed.ard and mixed.raw.shape == (9,) and torch.allclose(mixed.lengthscale, torch.full((3,), 0.8, dtype=F64), rtol=1e-14)
    # round trip; the raw period lengths are the LAST nls entries
    raw = torch.tensor([0.1, -1.0, 0.3, 0.2, 0.6, -0.4, 1.5, -0.7, 0.9], dtype=F64)
    assert torch.equal(model.set_raw_parameters(raw).raw_parameters(), raw)
    assert torch.allclose(model.lengthscale, sp(raw[3:6]), rtol=1e-15) and torch.allclose(model.period_length, sp(raw[6:9]), rtol=1e-15)
    lib = model._library_lengthscale()
    assert lib.shape == (1, 6) and torch.equal(lib[0, :3], model.lengthscale) and torch.equal(lib[0, 3:], model.period_length)
    with pytest.raises(AssertionError):
        model.set_raw_parameters(raw[:8])


def test_dirichlet_raw_layout():
    x, _ = _data(12, 2, 2)
    labels = torch.arange(12) % 3
    model = pkg.DirichletExactGP(x, labels, kernel=PeriodicKernel)
    assert model.kind == L.KERNEL_PERIODIC and model.raw.shape == (3, 7) and model.period_length.shape == (3, 2)
    raw = 0.3 * torch.randn(3, 7, generator=torch.Generator().manual_seed(4), dtype=F64)
    model.set_raw_parameters(raw)
    assert torch.equal(model.raw_parameters(), raw)
    assert torch.allclose(model.lengthscale, sp(raw[:, 3:5]), rtol=1e-15) and torch.allclose(model.period_length, sp(raw[:, 5:7]), rtol=1e-15)
    ls = model._library_lengthscale()
    assert ls.shape == (3, 4) and torch.equal(ls[:, :2], model.lengthscale) and torch.equal(ls[:, 2:], model.period_length)
    kernels = model.kernels
    assert [type(k) for k in kernels] == [PeriodicKernel] * 3
    assert all(torch.equal(k.period_length, model.period_length[c]) for c, k in enumerate(kernels))
    one = model.kernel  # the raw values averaged over the classes, softplus afterwards
    assert type(one) is PeriodicKernel and torch.allclose(one.period_length, sp(raw[:, 5:7].mean(dim=0)), rtol=1e-15)
    assert pkg.DirichletExactGP(x, labels, kernel=PeriodicKernel, ard=False).raw.shape == (3, 5)


def test_the_other_layouts_are_unchanged():
    x, y = _data(12, 3, 5)
    for kernel, width in (("rbf", 6), ("matern", 6), ("rq", 7), (ARDKernel([1.0]), 4), (RQKernel([1.0, 2.0, 3.0]), 7)):
        model = pkg.ExactGP(x, y, kernel=kernel)
        assert model.raw.shape == (width,) and not hasattr(model, "period_length")
        loss, grad = model.chain_rule(torch.arange(4 + 3 + (1 if model.kernel_name == "rq" else 0), dtype=F64))
        assert grad.shape == model.raw.shape and loss == 0.0
    for name in ("cosine", "periodic"):  # (the model classes take the class PeriodicKernel; the trainers take the name)
        with pytest.raises(ValueError, match="kernel must be one of"):
            pkg.ExactGP(x, y, kernel=name)
    for cls, name in ((ARDKernel, "rbf"), (RQKernel, "rq"), (pkg.MaternKernel, "matern")):
        assert pkg.ExactGP(x, y, kernel=cls).kernel_name == name and torch.equal(pkg.ExactGP(x, y, kernel=cls).raw.detach(),
                                                                                 pkg.ExactGP(x, y, kernel=name).raw.detach())
    with pytest.raises(TypeError, match="PeriodicKernel"):
        pkg.ExactGP(x, y, kernel=pkg.LinearKernel())


# ---- chain_rule against central differences ----------------------------------------------------------------------------
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_against_central_differences(ard):
    """chain_rule fed with the LAPACK helper's 4 + 2 d outputs against central differences of the helper's own value in every
    raw parameter, step h = 1e-5: truncation h^2 |f'''| / 6 = 2e-11 |f'''| and rounding eps |f| / h = 2e-11 |f|; n = 40 points
    with noise 0.127 keep |f| and |f'''| within 1e3 of the largest gradient component, so 1e-7 of that component is the bar."""
    x, y = _data(40, 3, 6)
    model = pkg.ExactGP(x, y, kernel=PeriodicKernel, ard=ard)
    g = torch.Generator().manual_seed(7 + ard)
    raw = 0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64)
    raw[1] = -2.0  # noise = 1e-4 + softplus(-2) = 0.127
    model.set_raw_parameters(raw)
    out, _ = T.mll_and_grad(x, y, model.lengthscale, model.period_length, model.outputscale, model.noise, model.mean_constant)
    assert out.shape == (4 + 6,)
    loss, grad = model.chain_rule(torch.from_numpy(out))
    assert grad.shape == raw.shape and loss == -out[0] / 40 and T.host_evaluate(model)[0] == loss

    def value(r):
        model.set_raw_parameters(r)
        return T.host_evaluate(model)[0]

    h = 1e-5
    want = torch.zeros_like(raw)
    for k in range(raw.numel()):
        step = torch.zeros_like(raw)
        step[k] = h
        want[k] = (value(raw + step) - value(raw - step)) / (2 * h)
    err = ((grad - want).abs().max() / want.abs().max()).item()
    nls = 3 if ard else 1
    print(f"{'ard' if ard else 'shared'}: gradient rel err {err:.2e}; d/d raw period {grad[3 + nls:].tolist()}")
    assert err <= 1e-7
    assert grad[3 + nls:].abs().min() > 1e-4 * want.abs().max(), "test construction: the period derivatives must matter"


def test_construct_average_ard_kernel_on_two_models():
    x, y = _data(12, 2, 8)
    a, b = pkg.ExactGP(x, y, kernel=PeriodicKernel), pkg.ExactGP(x, y, kernel=PeriodicKernel)
    a.set_raw_parameters(torch.tensor([0.0, 0.0, 0.2, 0.4, -0.6, 1.0, 0.5], dtype=F64))
    b.set_raw_parameters(torch.tensor([0.5, 0.1, 0.6, -0.2, 0.2, -2.0, 0.25], dtype=F64))
    k = pkg.construct_average_ard_kernel([a, b])
    assert type(k) is PeriodicKernel and k.outputscale == float(sp(torch.tensor(0.4, dtype=F64)))
    assert torch.equal(k.lengthscale, sp(torch.tensor([0.1, -0.2], dtype=F64)))
    assert torch.equal(k.period_length, sp(torch.tensor([-0.5, 0.375], dtype=F64)))
    shared = pkg.ExactGP(x, y, kernel=PeriodicKernel, ard=False)
    k = pkg.construct_average_ard_kernel([shared])
    assert type(k) is PeriodicKernel and k.lengthscale.numel() == 2 and k.period_length.numel() == 2
    assert torch.allclose(k.period_length, torch.full((2,), LN2, dtype=F64), rtol=1e-15)


def test_training_loop_and_runner_accept_periodic():
    """train_exact_gp with kernel=PeriodicKernel and with a PeriodicKernel instance, on the host evaluation"""
    x, y = _data(30, 2, 9)
    model, losses = pkg.train_exact_gp(x, y, "periodic", seed=1, number_of_epochs=5, learning_rate=0.05, early_stopper_patience=10.0,
                                       evaluate=T.host_evaluate)
    assert model.kind == L.KERNEL_PERIODIC and len(losses) == 5 and losses[-1] < losses[0]
    assert torch.all(model.raw_parameters()[5:] != 0.0), "the raw period lengths are learned"
    model, _ = pkg.train_exact_gp(x, y, PeriodicKernel([1.0, 2.0], 1.0, period_length=[1.3, 0.9]), seed=1, number_of_epochs=1,
                                  learning_rate=0.05, early_stopper_patience=10.0, evaluate=T.host_evaluate)
    assert model.kind == L.KERNEL_PERIODIC and model.raw.shape == (7,)
    model, _ = pkg.train_exact_gp(x, torch.arange(30) % 2, "periodic", seed=1, number_of_epochs=0, learning_rate=0.05,
                                  early_stopper_patience=10.0, likelihood="dirichlet")
    assert type(model) is pkg.DirichletExactGP and model.raw.shape == (2, 7)


# ---- the C ABI (validation only: no HIP call) ---------------------------------------------------------------------------
def test_cabi_accepts_the_kind_and_sizes_its_workspace():
    lib = L.load()
    p = 8  # (any non-NULL address: every call below fails its argument checks first)
    K = L.KERNEL_PERIODIC
    assert lib.pls_abi_version() == L.ABI_VERSION == 7 and K == 8
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 1, None, 1.0, p, 1, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(K, p, 4, 1, None, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, None, 1.0, 0.0, p, p, 3, p, None) == 1 and b"NULL pointer" in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, p, 1.0, 0.0, p, p, 0, p, None) == 0
    # 2 d + 1 sums and 4 + 2 d outputs
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5) == 8 * 11 * 2 * 9
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 130, 16) == 8 * 33 * 1 * 3
    assert lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3) == 8 * (7 * 5 * 6 + 2 * 6 + 8 + 8)  # v(7) = 8 twice
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 2) == lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 0) == 0
    # d = 17 is refused, by the queries with 0 and by every entry with the kind's own message; the other kinds keep 64
    msg = b"> 16 is not supported for the periodic kernel"
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 5, 17) == 0 and lib.pls_gp_mll_workspace_bytes_kind(K, 5, 17) == 0
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 17, 2) == 0 and lib.pls_gp_mll_workspace_bytes_kind(K, 5, 16) > 0
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 17, p, 1.0, p, 1, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 17, p, 1.0, 0.0, p, p, 3, p, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_kernel_grad_sums(K, p, 5, 17, p, 1.0, p, p, 5, p, 16, 1 << 20, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_gp_mll_grad(K, p, 5, 17, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, 1 << 20, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_gp_mll_grad_classes(K, p, 5, 17, 2, p, p, p, p, None, 5, p, 5, 0.0, p, p, 16, 1 << 20, None) == 1
    assert msg in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(K, p, 4, 17, p, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert msg in lib.pls_last_error()
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 65, p, 1.0, p, 1, None) == 1 and msg in lib.pls_last_error()
    for kind in (L.KERNEL_RBF_ARD, L.KERNEL_MATERN12, L.KERNEL_MATERN32, L.KERNEL_MATERN52, L.KERNEL_RQ):
        assert lib.pls_gp_mll_workspace_bytes_kind(kind, 5, 17) > 0 and lib.pls_gp_mll_workspace_bytes_kind(kind, 5, 64) > 0
        assert lib.pls_gp_mll_workspace_bytes_kind(kind, 5, 65) == 0
        assert lib.pls_kernel_gram(kind, p, 1, p, 1, 65, p, 1.0, p, 1, None) == 1
        assert b"> 64 is not supported" in lib.pls_last_error() and b"periodic" not in lib.pls_last_error()
    for kind in (L.KERNEL_RBF_ARD, L.KERNEL_MATERN52):  # the existing values stay
        for n, d in ((5, 3), (515, 5), (130, 64)):
            assert lib.pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d) == lib.pls_kernel_grad_sums_workspace_bytes(n, d)
            assert lib.pls_gp_mll_workspace_bytes_kind(kind, n, d) == lib.pls_gp_mll_workspace_bytes(n, d)
    # kinds 5, 7 and -1 are still unknown
    for bad in (5, 7, -1):
        assert lib.pls_gp_mll_workspace_bytes_kind(bad, 5, 3) == 0 and lib.pls_kernel_grad_sums_workspace_bytes_kind(bad, 5, 3) == 0
        assert lib.pls_kernel_gram(bad, p, 1, p, 1, 1, p, 1.0, p, 1, None) == 1 and b"unknown kernel kind" in lib.pls_last_error()
        assert lib.pls_kernel_mean(bad, p, 4, 2, p, 1.0, 0.0, p, p, 3, p, None) == 1 and b"unknown kernel kind" in lib.pls_last_error()
        assert lib.pls_gp_mll_grad(bad, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, 1 << 20, None) == 1
        assert b"unknown kernel kind" in lib.pls_last_error()
        assert lib.pls_select_inducing_conditional_variance(bad, p, 4, 1, p, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
        assert b"unknown kernel kind" in lib.pls_last_error()
    # the entries check against the kind-aware need: the RBF size is too small for 2 d + 1 sums
    old, need = lib.pls_gp_mll_workspace_bytes(5, 3), lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert need > old
    assert lib.pls_gp_mll_grad(K, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, old, None) == 3  # WORKSPACE_TOO_SMALL
    assert f"{need} needed".encode() in lib.pls_last_error()
    old, need = lib.pls_kernel_grad_sums_workspace_bytes(515, 5), lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5)
    assert lib.pls_kernel_grad_sums(K, p, 515, 5, p, 1.0, p, p, 515, p, 16, old, None) == 3
    assert f"{need} needed".encode() in lib.pls_last_error()
