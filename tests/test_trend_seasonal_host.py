"""CPU: the host side of the trend-plus-seasonal base kernel (RBF + RBF x periodic) -- the closed-form yardstick against
50-digit arithmetic (three whole evaluations), the kernel class, ``prior_variance`` for every family, the gpytorch-shaped sum
that as_base_kernel reads, the raw parameter layout of ExactGP / DirichletExactGP with FOUR shape blocks behind the raw
lengthscales (three per dimension and one scalar), chain_rule against central differences, the averaging constructor, and the
C ABI's argument checks and kind-aware workspace queries (they run before any HIP call)."""
import numpy as np
import pytest
import torch

import projected_langevin_sampling_amd as pkg
import trend_seasonal_truth as T
from locally_periodic_closed_form import LN2, locally_periodic_numpy
from projected_langevin_sampling_amd.kernel import (ARDKernel, LocallyPeriodicKernel, MaternKernel, PeriodicKernel, RQKernel,
                                                    TrendSeasonalKernel, as_base_kernel)
from trend_seasonal_closed_form import trend_seasonal_factors_numpy, trend_seasonal_numpy, trend_seasonal_torch

L = pkg._lib
F64 = torch.float64
sp = torch.nn.functional.softplus
BLOCKS = ("lengthscale", "seasonal_lengthscale", "periodic_lengthscale", "period_length")


# ---- the yardstick -------------------------------------------------------------------------------------------------------
def test_closed_forms_agree_and_hold_the_diagonal():
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(7, 3, generator=g, dtype=F64), torch.randn(9, 3, generator=g, dtype=F64)
    ls, env = 2.0 + torch.rand(3, generator=g, dtype=F64), 1.0 + torch.rand(3, generator=g, dtype=F64)
    lam, period = 0.5 + torch.rand(3, generator=g, dtype=F64), 0.5 + 2.5 * torch.rand(3, generator=g, dtype=F64)
    kt = trend_seasonal_torch(ls, 2.5, env, lam, period, 0.9)
    kn = trend_seasonal_numpy(ls.numpy(), 2.5, env.numpy(), lam.numpy(), period.numpy(), 0.9)
    a, b = kt(x1, x2).numpy(), kn(x1.numpy(), x2.numpy())
    assert np.abs(a - b).max() <= 16 * T.EPS * 3.4  # (the exponents are O(1) here: a few eps from each library)
    assert np.all(kt(x1, x1).diagonal().numpy() == 2.5 + 0.9) and np.all(np.diag(kn(x1.numpy(), x1.numpy())) == 2.5 + 0.9)
    far = torch.full((1, 3), float("inf"), dtype=F64)
    assert torch.isnan(kt(far, -far)).all() and np.isnan(kn(far.numpy(), -far.numpy())).all(), "a non-finite difference: NaN"
    # the sum of the two terms it is made of
    rbf = 2.5 * np.exp(-0.5 * np.square((x1.numpy()[:, None, :] - x2.numpy()[None, :, :]) / ls.numpy()).sum(-1))
    seasonal = locally_periodic_numpy(env.numpy(), 0.9, lam.numpy(), period.numpy())(x1.numpy(), x2.numpy())
    assert np.abs(b - (rbf + seasonal)).max() <= 4 * T.EPS * 3.4


@pytest.mark.parametrize("name", list(T.CASES))
def test_lapack_helper_is_a_legitimate_yardstick(name):
    """trend_seasonal_truth.mll_and_grad against the 50-digit truth, per output relative to its sum-of-magnitudes scale S.
    The GPU bar of test_gpu_trend_seasonal is max(16 e_cpu, 64 eps); the helper's own error must be at most 1/16 of it.
    That alone holds by construction, so the helper is also held to what a backward-stable Cholesky evaluation can show:
    n cond(K_y) eps relative to S (Higham, Accuracy and Stability, thm. 10.4 with the growth factor n)."""
    x, y, ls, env, lam, period = T.case_inputs(name)
    n, d = x.shape
    out, mag, e_cpu = T.cpu_case(name)
    assert out.shape == mag.shape == (4 + 4 * d + 1,) and np.all(mag > 0)
    gpu_bar = np.maximum(16.0 * e_cpu, 64.0 * T.EPS)
    k = T.gram(x, ls, env, lam, period, T.S_T, T.S_S)
    cond = torch.linalg.cond(k + T.NOISE * torch.eye(n, dtype=F64)).item()
    print(f"{name}: e_cpu max {e_cpu.max():.2e} = {e_cpu.max() / T.EPS:.1f} eps, cond(K_y) {cond:.1e}, per output " +
          " ".join(f"{v / T.EPS:.1f}" for v in e_cpu))
    assert np.all(e_cpu <= gpu_bar / 16.0) and np.all(e_cpu <= n * cond * T.EPS)
    assert (k > 1e-3 * (T.S_T + T.S_S)).double().mean().item() >= 0.5, "test construction: most entries must be of the size of s"
    assert torch.all(ls > env), "test construction: the trend is longer than the envelope"


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8])
def test_the_draws_keep_the_entries_of_the_size_of_s(d):
    """the draws of the GPU file (x ~ N(0, I), l = (2 + U) sqrt(d), m, lambda, p as the locally periodic file's, s_t = 2.5,
    s_s = 0.9): on (65, 515) at least half of the entries of the closed form exceed 1e-3 (s_t + s_s), and the seasonal term
    is no rounding error beside the trend -- so the GPU file's construction asserts rest on the reference alone"""
    g = torch.Generator().manual_seed(2000 * d + 12)
    x1, x2 = torch.randn(65, d, generator=g, dtype=F64), torch.randn(515, d, generator=g, dtype=F64)
    ls, env, lam, period = T.draw_parameters(g, d)
    f = trend_seasonal_factors_numpy(x1.numpy()[:, None, :] - x2.numpy()[None, :, :], ls.numpy(), env.numpy(), lam.numpy(),
                                     period.numpy())
    k = T.S_T * f[0] + T.S_S * f[2]
    share = float((k > 1e-3 * (T.S_T + T.S_S)).mean())
    seasonal = float((T.S_S * f[2] > 1e-3 * k).mean())
    print(f"d={d}: {share:.3f} of the entries above 1e-3 (s_t + s_s), the seasonal term above 1e-3 of the entry in {seasonal:.3f}")
    assert share >= 0.5 and seasonal >= 0.5


# ---- kernel objects ------------------------------------------------------------------------------------------------------
def _stub(**attributes):
    return type("Stub", (), attributes)()


def _sum_stub(*members):
    return _stub(kernels=list(members))


def test_kernel_class_and_validation():
    k = TrendSeasonalKernel([3.0, 4.0, 5.0], 2.5, seasonal_lengthscale=[0.5, 2.0, 1.25], periodic_lengthscale=[0.9, 1.1, 0.6],
                            period_length=[1.0, 0.7, 2.5], seasonal_outputscale=0.9)
    assert k.kind == L.KERNEL_TREND_SEASONAL == T.TREND_SEASONAL == 12 and k.outputscale == 2.5 and k.family == "trend_seasonal"
    assert k.seasonal_outputscale == 0.9 and isinstance(k.seasonal_outputscale, float)
    assert k.lengthscale.tolist() == [3.0, 4.0, 5.0] and k.seasonal_lengthscale.tolist() == [0.5, 2.0, 1.25]
    assert k.periodic_lengthscale.tolist() == [0.9, 1.1, 0.6] and k.period_length.tolist() == [1.0, 0.7, 2.5]
    assert k._lengthscale_host(3).tolist() == [3.0, 4.0, 5.0, 0.5, 2.0, 1.25, 0.9, 1.1, 0.6, 1.0, 0.7, 2.5, 0.9], "l, m, lambda, p, s_s"
    shared = TrendSeasonalKernel([3.0], 1.5, seasonal_lengthscale=0.75, periodic_lengthscale=0.5, period_length=2.0,
                                 seasonal_outputscale=torch.tensor([0.25]))
    assert shared._lengthscale_host(4).tolist() == [3.0] * 4 + [0.75] * 4 + [0.5] * 4 + [2.0] * 4 + [0.25]
    default = TrendSeasonalKernel([1.0])
    assert default.outputscale == default.seasonal_outputscale == 1.0 and default._lengthscale_host(1).tolist() == [1.0] * 5
    assert pkg.TrendSeasonalKernel is TrendSeasonalKernel and "TrendSeasonalKernel" in pkg.__all__
    from projected_langevin_sampling_amd.kernel import STATIONARY_KERNEL_NAMES, STATIONARY_KERNELS, _StationaryKernel
    assert isinstance(k, _StationaryKernel) and STATIONARY_KERNELS[-1] is TrendSeasonalKernel
    assert STATIONARY_KERNEL_NAMES.endswith("LocallyPeriodicKernel / TrendSeasonalKernel")
    assert TrendSeasonalKernel.shape_blocks == (("seasonal_lengthscale", True), ("periodic_lengthscale", True),
                                                ("period_length", True), ("seasonal_outputscale", False))
    assert TrendSeasonalKernel.keyword is None
    for bad in (0.0, -1.0, [1.0, 0.0], float("nan")):
        with pytest.raises(ValueError, match="every period length"):
            TrendSeasonalKernel([1.0, 1.0], 1.0, period_length=bad)
        with pytest.raises(ValueError, match="every periodic lengthscale"):
            TrendSeasonalKernel([1.0, 1.0], 1.0, periodic_lengthscale=bad)
        with pytest.raises(ValueError, match="every seasonal lengthscale"):
            TrendSeasonalKernel([1.0, 1.0], 1.0, seasonal_lengthscale=bad)
        with pytest.raises(ValueError, match="every lengthscale"):
            TrendSeasonalKernel(bad, 1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="every seasonal outputscale"):
            TrendSeasonalKernel([1.0, 1.0], 1.0, seasonal_outputscale=bad)
    with pytest.raises(AssertionError, match="has 3 entries, data has 2 dims"):
        k._lengthscale_host(2)


def test_prior_variance_of_every_family():
    """k(x, x): the outputscale for every family with one term, the sum of the two here -- fl(s_t + s_s), what the library's
    fma gives on the diagonal"""
    assert ARDKernel([1.0], 1.7).prior_variance == 1.7 and MaternKernel([1.0], 0.3, nu=1.5).prior_variance == 0.3
    assert RQKernel([1.0], 2.0, alpha=0.5).prior_variance == 2.0 and PeriodicKernel([1.0], 1.1).prior_variance == 1.1
    assert LocallyPeriodicKernel([1.0], 0.7).prior_variance == 0.7
    k = TrendSeasonalKernel([1.0], 2.5, seasonal_outputscale=0.9)
    assert k.prior_variance == 2.5 + 0.9 and isinstance(k.prior_variance, float)
    assert TrendSeasonalKernel([1.0], 0.1, seasonal_outputscale=0.2).prior_variance == 0.1 + 0.2 != 0.3
    with pytest.raises(AttributeError):
        k.prior_variance = 1.0


def test_as_base_kernel_reads_the_sum():
    rbf = _stub(base_kernel=_stub(lengthscale=torch.tensor([[3.0, 4.0, 5.0]])), outputscale=torch.tensor(2.5))
    envelope = _stub(lengthscale=torch.tensor([[0.5, 2.0, 1.25]]))
    periodic = _stub(lengthscale=torch.tensor([[0.875, 1.125, 0.625]]), period_length=torch.tensor([[1.0, 0.75, 2.5]]))  # (float32-exact)
    seasonal = _stub(base_kernel=_stub(kernels=[periodic, envelope]), outputscale=torch.tensor(0.75))
    for members in ((rbf, seasonal), (seasonal, rbf)):  # either order
        k = as_base_kernel(_sum_stub(*members))
        assert type(k) is TrendSeasonalKernel and k.outputscale == 2.5 and k.seasonal_outputscale == 0.75
        assert k._lengthscale_host(3).tolist() == [3.0, 4.0, 5.0, 0.5, 2.0, 1.25, 0.875, 1.125, 0.625, 1.0, 0.75, 2.5, 0.75]
    assert as_base_kernel(k) is k
    # every other sum is refused with the existing TypeError
    matern = _stub(base_kernel=_stub(lengthscale=torch.tensor([[1.0]]), nu=2.5), outputscale=1.0)
    plain_periodic = _stub(base_kernel=periodic, outputscale=1.0)
    for members in ((rbf, rbf), (seasonal, seasonal), (rbf,), (rbf, seasonal, rbf), (rbf, plain_periodic), (matern, seasonal),
                    (rbf, envelope), (rbf, _stub(base_kernel=_stub(kernels=[envelope, envelope]), outputscale=1.0)),
                    (rbf, _stub(base_kernel=_stub(kernels=[periodic, envelope])))):
        with pytest.raises(TypeError, match="unsupported base kernel"):
            as_base_kernel(_sum_stub(*members))
    # the single-kernel and the product readings are as they were
    assert type(as_base_kernel(rbf)) is ARDKernel and type(as_base_kernel(seasonal)) is LocallyPeriodicKernel
    assert type(as_base_kernel(plain_periodic)) is PeriodicKernel


# ---- the raw layout ------------------------------------------------------------------------------------------------------
def _data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.sin(x.sum(dim=1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)


def _start():
    return TrendSeasonalKernel([3.0, 4.0, 5.0], 1.7, seasonal_lengthscale=[0.5, 2.0, 1.25], periodic_lengthscale=[0.9, 1.1, 0.6],
                               period_length=[1.0, 0.7, 2.5], seasonal_outputscale=0.6)


def test_exact_gp_raw_layout_and_start_values():
    x, y = _data(12, 3, 1)
    model = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel)
    assert model.kind == L.KERNEL_TREND_SEASONAL and model.kernel_name == "trend_seasonal" and model.raw.shape == (16,)  # 3 + 4 nls + 1
    assert torch.equal(model.raw.detach(), torch.zeros(16, dtype=F64))
    for name in BLOCKS:
        values = getattr(model, name)
        assert values.shape == (3,) and torch.allclose(values, torch.full((3,), LN2, dtype=F64), rtol=1e-15)
    assert model.seasonal_outputscale == pytest.approx(LN2, rel=1e-15) and isinstance(model.seasonal_outputscale, float)
    assert not hasattr(model, "alpha") and not hasattr(pkg.ExactGP(x, y, kernel="rbf"), "seasonal_lengthscale")
    assert not hasattr(pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel), "seasonal_outputscale")
    shared = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel, ard=False)
    assert shared.raw.shape == (8,), "3 + 1 + 4 columns"
    assert shared.period_length.shape == (3,) and shared.seasonal_lengthscale.shape == (3,) and shared._library_lengthscale().shape == (1, 13)
    start = _start()
    model = pkg.ExactGP(x, y, kernel=start)
    assert model.kind == L.KERNEL_TREND_SEASONAL and model.ard and model.raw.shape == (16,)
    # the round trip start kernel -> raw -> library values
    assert torch.allclose(model._library_lengthscale()[0], start._lengthscale_host(3), rtol=1e-14)
    for name in BLOCKS:
        assert torch.allclose(getattr(model, name), getattr(start, name), rtol=1e-14), name
    assert model.outputscale == pytest.approx(1.7, rel=1e-14) and model.seasonal_outputscale == pytest.approx(0.6, rel=1e-14)
    fitted = model.kernel
    assert type(fitted) is TrendSeasonalKernel and fitted.outputscale == model.outputscale
    assert fitted.seasonal_outputscale == model.seasonal_outputscale
    assert fitted.prior_variance == model.outputscale + model.seasonal_outputscale
    assert all(torch.equal(getattr(fitted, name), getattr(model, name)) for name in BLOCKS)
    assert torch.equal(fitted._lengthscale_host(3), model._library_lengthscale()[0])
    one = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel([2.8], 1.1, seasonal_lengthscale=[0.8], periodic_lengthscale=[0.6],
                                                       period_length=[1.3], seasonal_outputscale=0.4))
    assert not one.ard and one.raw.shape == (8,)
    assert torch.allclose(one._library_lengthscale()[0], torch.tensor([2.8] * 3 + [0.8] * 3 + [0.6] * 3 + [1.3] * 3 + [0.4], dtype=F64),
                          rtol=1e-14)
    for mixed in (TrendSeasonalKernel([2.8], 1.1, period_length=[1.0, 0.7, 2.5]),
                  TrendSeasonalKernel([2.8], 1.1, seasonal_lengthscale=[1.0, 0.7, 2.5])):  # a per-dimension block: ard
        model2 = pkg.ExactGP(x, y, kernel=mixed)
        assert model2.ard and model2.raw.shape == (16,)
        assert torch.allclose(model2._library_lengthscale()[0], mixed._lengthscale_host(3), rtol=1e-14)
    # the raw order: l, m, lambda, p, s_s
    raw = torch.tensor([0.1, -1.0, 0.3, 0.2, 0.6, -0.4, 1.5, -0.7, 0.9, -0.3, 0.8, 0.05, 0.45, -0.15, 0.35, -0.9], dtype=F64)
    assert torch.equal(model.set_raw_parameters(raw).raw_parameters(), raw)
    for b, name in enumerate(BLOCKS):
        assert torch.allclose(getattr(model, name), sp(raw[3 + 3 * b:6 + 3 * b]), rtol=1e-15), name
    assert model.seasonal_outputscale == pytest.approx(float(sp(raw[15])), rel=1e-15)
    lib = model._library_lengthscale()
    assert lib.shape == (1, 13) and all(torch.equal(lib[0, 3 * b:3 * b + 3], getattr(model, name)) for b, name in enumerate(BLOCKS))
    assert lib[0, 12].item() == model.seasonal_outputscale
    with pytest.raises(AssertionError):
        model.set_raw_parameters(raw[:15])


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_widths_follow_the_library_count(ard):
    """the width checks of test_kernel_family_host.py for the family with four blocks: _lengthscale_host,
    _library_lengthscale, the raw width and the chain_rule shape, tied to the library's own count through the workspace query"""
    d = 3
    lib = L.load()
    for n, dd in ((515, 5), (130, 8)):
        blocks = -(-n // 512) * -(-n // 64)
        assert lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_TREND_SEASONAL, n, dd) == 8 * blocks * (4 * dd + 2)
        assert L.kernel_shape_params(L.KERNEL_TREND_SEASONAL, dd) == 3 * dd + 1
    x, y = _data(10, d, 3)
    kernel = _start() if ard else TrendSeasonalKernel([3.0], 1.3, seasonal_lengthscale=0.5, periodic_lengthscale=0.9,
                                                      period_length=1.5, seasonal_outputscale=0.6)
    assert kernel._lengthscale_host(d).numel() == 4 * d + 1
    model = pkg.ExactGP(x, y, kernel=kernel, ard=ard)
    nls = d if ard else 1
    assert model.raw.numel() == 3 + 4 * nls + 1 == 3 + nls + L.kernel_shape_params(model.kind, nls)
    assert model._library_lengthscale().shape == (1, 4 * d + 1)
    assert torch.allclose(model._library_lengthscale()[0], kernel._lengthscale_host(d), rtol=1e-14)
    loss, grad = model.chain_rule(torch.arange(4 + 4 * d + 1, dtype=F64))
    assert grad.shape == model.raw.shape and loss == 0.0
    assert type(model.kernel) is TrendSeasonalKernel and model.kernel._lengthscale_host(d).numel() == 4 * d + 1


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_sums_block_by_block(ard):
    """chain_rule fed an ``out`` whose entries are known: out[4 + j] = (j + 1) v_j with v the library's natural values, so that
    d/d natural value j is j + 1.  Per dimension, raw column c of a block gets (j + 1) sigmoid(raw); a shared raw column gets
    the sum of ITS OWN block's d entries and nothing of its neighbours'; the scalar block behind them gets its one entry."""
    d, n = 3, 10
    x, y = _data(n, d, 4)
    model = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel, ard=ard)
    nls = d if ard else 1
    raw = 0.5 * torch.randn(3 + 4 * nls + 1, generator=torch.Generator().manual_seed(5), dtype=F64)
    model.set_raw_parameters(raw)
    natural = model._library_lengthscale()[0]
    out = torch.zeros(4 + 4 * d + 1, dtype=F64)
    out[4:] = torch.arange(1, 4 * d + 2, dtype=F64) * natural
    _, grad = model.chain_rule(out)
    slope = torch.sigmoid(raw)
    for block in range(4):
        weights = torch.arange(1 + block * d, 1 + (block + 1) * d, dtype=F64)
        columns = slice(3 + block * nls, 3 + (block + 1) * nls)
        want = (weights if ard else weights.sum(dim=0, keepdim=True)) * slope[columns]
        assert torch.allclose(grad[columns], -want / n, rtol=1e-14), (block, grad[columns], -want / n)
    assert torch.allclose(grad[-1], -(4 * d + 1) * slope[-1] / n, rtol=1e-14)
    assert torch.equal(grad[:3], torch.zeros(3, dtype=F64))


def test_dirichlet_raw_layout():
    x, _ = _data(12, 2, 2)
    labels = torch.arange(12) % 3
    model = pkg.DirichletExactGP(x, labels, kernel=TrendSeasonalKernel)
    assert model.kind == L.KERNEL_TREND_SEASONAL and model.raw.shape == (3, 12) and model.period_length.shape == (3, 2)
    assert model.seasonal_lengthscale.shape == (3, 2) and model.seasonal_outputscale.shape == (3,)
    raw = 0.3 * torch.randn(3, 12, generator=torch.Generator().manual_seed(4), dtype=F64)
    model.set_raw_parameters(raw)
    assert torch.equal(model.raw_parameters(), raw)
    for b, name in enumerate(BLOCKS):
        assert torch.allclose(getattr(model, name), sp(raw[:, 3 + 2 * b:5 + 2 * b]), rtol=1e-15), name
    assert torch.allclose(model.seasonal_outputscale, sp(raw[:, 11]), rtol=1e-15)
    ls = model._library_lengthscale()
    assert ls.shape == (3, 9) and torch.equal(ls[:, 8], model.seasonal_outputscale)
    kernels = model.kernels
    assert [type(k) for k in kernels] == [TrendSeasonalKernel] * 3
    assert all(torch.equal(k._lengthscale_host(2), ls[c]) for c, k in enumerate(kernels))
    one = model.kernel  # the raw values averaged over the classes, softplus afterwards
    assert type(one) is TrendSeasonalKernel and torch.allclose(one.period_length, sp(raw[:, 9:11].mean(dim=0)), rtol=1e-15)
    assert one.seasonal_outputscale == pytest.approx(float(sp(raw[:, 11].mean())), rel=1e-15)
    assert pkg.DirichletExactGP(x, labels, kernel=TrendSeasonalKernel, ard=False).raw.shape == (3, 8)


def test_the_names_the_model_classes_and_the_trainers_take():
    x, y = _data(12, 3, 5)
    with pytest.raises(ValueError, match="kernel must be one of"):  # (the model classes take the class; the trainers the name)
        pkg.ExactGP(x, y, kernel="trend_seasonal")
    with pytest.raises(TypeError, match="a TrendSeasonalKernel"):
        pkg.ExactGP(x, y, kernel=pkg.LinearKernel())
    from projected_langevin_sampling_amd.inducing_point_selectors import ConditionalVarianceInducingPointSelector
    with pytest.raises(TypeError, match="TrendSeasonalKernel"):
        ConditionalVarianceInducingPointSelector()(x, 4, _stub(kernels=[]))


# ---- chain_rule against central differences ----------------------------------------------------------------------------
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_against_central_differences(ard):
    """chain_rule fed with the LAPACK helper's 4 + 4 d + 1 outputs against central differences of the helper's own value in
    every raw parameter, step h = 1e-5, with the periodic host test's bar (1e-7 of the largest gradient component: truncation
    h^2 |f'''| / 6 and rounding eps |f| / h are both 2e-11 of |f'''| and |f|)."""
    x, y = _data(40, 3, 6)
    model = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel, ard=ard)
    g = torch.Generator().manual_seed(7 + ard)
    raw = 0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64)
    raw[1] = -2.0  # noise = 1e-4 + softplus(-2) = 0.127
    model.set_raw_parameters(raw)
    out, _ = T.mll_and_grad(x, y, model.lengthscale, model.seasonal_lengthscale, model.periodic_lengthscale, model.period_length,
                            model.outputscale, model.seasonal_outputscale, model.noise, model.mean_constant)
    assert out.shape == (4 + 13,)
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
    print(f"{'ard' if ard else 'shared'}: gradient rel err {err:.2e}; d/d raw {grad.tolist()}")
    assert err <= 1e-7
    assert grad[2:].abs().min() > 1e-4 * want.abs().max(), "test construction: every block's derivatives must matter"


def test_construct_average_ard_kernel_on_two_models():
    x, y = _data(12, 2, 8)
    a, b = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel), pkg.ExactGP(x, y, kernel=TrendSeasonalKernel)
    a.set_raw_parameters(torch.tensor([0.0, 0.0, 0.2, 0.4, -0.6, 1.0, 0.5, 0.25, -1.0, 0.5, 1.5, -0.5], dtype=F64))
    b.set_raw_parameters(torch.tensor([0.5, 0.1, 0.6, -0.2, 0.2, -2.0, 0.25, 0.75, 2.0, 0.0, -0.5, 1.0], dtype=F64))
    k = pkg.construct_average_ard_kernel([a, b])
    assert type(k) is TrendSeasonalKernel and k.outputscale == float(sp(torch.tensor(0.4, dtype=F64)))
    assert torch.equal(k.lengthscale, sp(torch.tensor([0.1, -0.2], dtype=F64)))
    assert torch.equal(k.seasonal_lengthscale, sp(torch.tensor([-0.5, 0.375], dtype=F64))), "every block is averaged"
    assert torch.equal(k.periodic_lengthscale, sp(torch.tensor([0.5, 0.5], dtype=F64)))
    assert torch.equal(k.period_length, sp(torch.tensor([0.25, 0.5], dtype=F64)))
    assert k.seasonal_outputscale == float(sp(torch.tensor(0.25, dtype=F64)))
    shared = pkg.ExactGP(x, y, kernel=TrendSeasonalKernel, ard=False)
    k = pkg.construct_average_ard_kernel([shared])
    assert type(k) is TrendSeasonalKernel and all(getattr(k, name).numel() == 2 for name in BLOCKS)
    assert torch.allclose(k._lengthscale_host(2), torch.full((9,), LN2, dtype=F64), rtol=1e-15)


def test_training_loop_and_runner_accept_the_name():
    """train_exact_gp with kernel="trend_seasonal", with the class and with an instance, on the host evaluation"""
    x, y = _data(30, 2, 9)
    args = dict(seed=1, learning_rate=0.05, early_stopper_patience=10.0)
    model, losses = pkg.train_exact_gp(x, y, "trend_seasonal", number_of_epochs=5, evaluate=T.host_evaluate, **args)
    assert model.kind == L.KERNEL_TREND_SEASONAL and len(losses) == 5 and losses[-1] < losses[0]
    assert torch.all(model.raw_parameters()[2:] != 0.0), "both outputscales and all four blocks are learned"
    by_class, losses2 = pkg.train_exact_gp(x, y, TrendSeasonalKernel, number_of_epochs=5, evaluate=T.host_evaluate, **args)
    assert losses2 == losses and torch.equal(by_class.raw_parameters(), model.raw_parameters())
    start = TrendSeasonalKernel([3.0, 2.0], 1.0, seasonal_lengthscale=[1.0, 2.0], periodic_lengthscale=[0.7, 1.2],
                                period_length=[1.3, 0.9], seasonal_outputscale=0.5)
    model, _ = pkg.train_exact_gp(x, y, start, number_of_epochs=1, evaluate=T.host_evaluate, **args)
    assert model.kind == L.KERNEL_TREND_SEASONAL and model.raw.shape == (12,)
    model, _ = pkg.train_exact_gp(x, torch.arange(30) % 2, "trend_seasonal", number_of_epochs=0, likelihood="dirichlet", **args)
    assert type(model) is pkg.DirichletExactGP and model.raw.shape == (2, 12)


# ---- the C ABI (validation only: no HIP call) ---------------------------------------------------------------------------
def test_cabi_accepts_the_kind_and_sizes_its_workspace():
    lib = L.load()
    p = 8  # (any non-NULL address: every call below fails its argument checks first)
    K = L.KERNEL_TREND_SEASONAL
    assert lib.pls_abi_version() == L.ABI_VERSION == 7 and K == 12
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 1, None, 1.0, p, 1, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(K, p, 4, 1, None, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, None, 1.0, 0.0, p, p, 3, p, None) == 1 and b"NULL pointer" in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, p, 1.0, 0.0, p, p, 0, p, None) == 0
    # 4 d + 2 sums and 4 + 4 d + 1 outputs
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5) == 8 * 22 * 2 * 9
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 130, 8) == 8 * 34 * 1 * 3
    assert lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3) > lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_LOCALLY_PERIODIC, 5, 3)
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 2) == lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 0) == 0
    # d = 9 is refused, by the queries with 0 and by every entry with the kind's own message
    msg = b"> 8 is not supported for the trend-plus-seasonal kernel"
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 5, 9) == 0 and lib.pls_gp_mll_workspace_bytes_kind(K, 5, 9) == 0
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 9, 2) == 0 and lib.pls_gp_mll_workspace_bytes_kind(K, 5, 8) > 0
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 9, p, 1.0, p, 1, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 9, p, 1.0, 0.0, p, p, 3, p, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_kernel_grad_sums(K, p, 5, 9, p, 1.0, p, p, 5, p, 16, 1 << 20, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_gp_mll_grad(K, p, 5, 9, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, 1 << 20, None) == 1 and msg in lib.pls_last_error()
    assert lib.pls_gp_mll_grad_classes(K, p, 5, 9, 2, p, p, p, p, None, 5, p, 5, 0.0, p, p, 16, 1 << 20, None) == 1
    assert msg in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(K, p, 4, 9, p, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert msg in lib.pls_last_error()
    # the locally periodic kind keeps its own limit and message
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_LOCALLY_PERIODIC, 5, 16) > 0
    assert lib.pls_kernel_gram(L.KERNEL_LOCALLY_PERIODIC, p, 1, p, 1, 17, p, 1.0, p, 1, None) == 1
    assert b"> 16 is not supported for the locally periodic kernel" in lib.pls_last_error()
    # kinds 9 and 11 are still refused as unknown
    for bad in (9, 11, 13):
        unknown = f"unknown kernel kind {bad}".encode()
        assert lib.pls_gp_mll_workspace_bytes_kind(bad, 5, 3) == 0 and lib.pls_kernel_grad_sums_workspace_bytes_kind(bad, 5, 3) == 0
        assert lib.pls_gp_mll_classes_workspace_bytes_kind(bad, 5, 3, 2) == 0
        assert lib.pls_kernel_gram(bad, p, 1, p, 1, 1, p, 1.0, p, 1, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_kernel_mean(bad, p, 4, 2, p, 1.0, 0.0, p, p, 3, p, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_kernel_grad_sums(bad, p, 5, 3, p, 1.0, p, p, 5, p, 16, 1 << 20, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_gp_mll_grad(bad, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, 1 << 20, None) == 1
        assert unknown in lib.pls_last_error()
        assert lib.pls_select_inducing_conditional_variance(bad, p, 4, 1, p, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
        assert unknown in lib.pls_last_error()
    # the entries check against the kind-aware need: a workspace sized for the locally periodic kind is too small
    old, need = lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_LOCALLY_PERIODIC, 5, 3), lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert lib.pls_gp_mll_grad(K, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, old, None) == 3  # WORKSPACE_TOO_SMALL
    assert f"{need} needed".encode() in lib.pls_last_error()
    old = lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_LOCALLY_PERIODIC, 515, 5)
    need = lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5)
    assert lib.pls_kernel_grad_sums(K, p, 515, 5, p, 1.0, p, p, 515, p, 16, old, None) == 3
    assert f"{need} needed".encode() in lib.pls_last_error()
