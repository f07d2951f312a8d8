"""CPU: the host side of the locally periodic base kernel (RBF envelope x periodic) -- the closed-form yardstick against
50-digit arithmetic (a per-pair table and three whole evaluations), the kernel class and the gpytorch-shaped product that
as_base_kernel reads, the raw parameter layout of ExactGP / DirichletExactGP with TWO shape blocks behind the raw
lengthscales, chain_rule block by block, the averaging constructor, and the C ABI's argument checks and kind-aware workspace
queries (they run before any HIP call)."""
import numpy as np
import pytest
import torch

import locally_periodic_truth as T
import projected_langevin_sampling_amd as pkg
from locally_periodic_closed_form import LN2, locally_periodic_factors_numpy, locally_periodic_numpy, locally_periodic_torch
from projected_langevin_sampling_amd.kernel import ARDKernel, LocallyPeriodicKernel, PeriodicKernel, as_base_kernel

L = pkg._lib
F64 = torch.float64
sp = torch.nn.functional.softplus


# ---- the yardstick -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(T.PAIR_PERIODS)), ids=[f"p={p:g}" for p in T.PAIR_PERIODS])
def test_numpy_helper_against_50_digits(k):
    """kappa, fe, fl and fp of locally_periodic_factors_numpy per pair of the fixture's table.  Bars from the formulas, the
    periodic host test's with the envelope added.  The reduced angle theta = pi r carries dth = (pi |e| / 2 + pi / 2) eps
    absolute (the rounding of e = delta / p, absent for the power-of-two periods, and of pi r with the sine and cosine near
    pi / 2).  fe = fl(fl(delta / l)^2) carries 3/2 eps relative; with q = fe / 2 + fl the negated exponent:
        kappa: (3 q + 8) eps kappa + kappa (2 / lambda) dth
        fe:    4 fe eps
        fl:    8 fl eps + (2 / lambda) dth
        fp:    8 |fp| eps + (2 / lambda) pi |e| (2 dth + eps / 2)          (the last: e itself, in front)
    The pair at e = 1000.25 is dead for p = 1 and 0.7 (exponent below -745.2): its kappa is exactly 0."""
    p, lam, ls = T.PAIR_PERIODS[k], T.PAIR_PERIODIC_LENGTHSCALE, T.PAIR_LENGTHSCALE
    hi, lo = T.pair_truth()
    delta = T.pair_deltas()[k]
    kap, fe, fl, fp, e = locally_periodic_factors_numpy(delta[:, None], [ls], [lam], [p])
    fe, fl, fp, e = fe[:, 0], fl[:, 0], fp[:, 0], e[:, 0]
    inexact = 0.0 if p != 0.7 else 1.0  # (p = 1 and 2^-3: the quotient and its reduction are exact)
    dth = (np.pi * np.abs(e) * 0.5 * inexact + np.pi / 2.0) * T.EPS
    q = 0.5 * fe + fl
    bars = {"kappa": (3.0 * q + 8.0) * T.EPS * hi[k, 0] + hi[k, 0] * (2.0 / lam) * dth,
            "fe": 4.0 * hi[k, 1] * T.EPS,
            "fl": 8.0 * hi[k, 2] * T.EPS + (2.0 / lam) * dth,
            "fp": 8.0 * np.abs(hi[k, 3]) * T.EPS + (2.0 / lam) * np.pi * np.abs(e) * (2.0 * dth + 0.5 * T.EPS * inexact)}
    for row, (name, got) in enumerate((("kappa", kap), ("fe", fe), ("fl", fl), ("fp", fp))):
        err = np.abs((got - hi[k, row]) - lo[k, row])
        bar = bars[name] + 1e-300  # (the floor: entries that are subnormal or 0)
        print(f"p={p:g} {name}: max err/bar {np.max(err / bar):.3f}")
        assert np.all(err <= bar), (name, err / bar)
    assert kap[0] == 1.0 and fe[0] == 0.0 and fl[0] == 0.0 and fp[0] == 0.0, "distance 0: kappa = 1 and all factors 0 exactly"
    whole = T.PAIR_E == 1.0
    assert np.all(kap[whole] < 1.0) and np.all(hi[k, 0][whole] < 1.0), "a whole period apart the envelope keeps kappa below 1"
    if p != 2.0**-3:
        dead = T.PAIR_E == 1000.25
        assert np.all(kap[dead] == 0.0) and np.all(hi[k, 0][dead] == 0.0), "(1000 / 3)^2 / 2 > 745.2: a dead pair"


def test_closed_forms_agree_and_hold_the_diagonal():
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(7, 3, generator=g, dtype=F64), torch.randn(9, 3, generator=g, dtype=F64)
    ls, lam = 1.0 + torch.rand(3, generator=g, dtype=F64), 0.5 + torch.rand(3, generator=g, dtype=F64)
    period = 0.5 + 2.5 * torch.rand(3, generator=g, dtype=F64)
    kt, kn = locally_periodic_torch(ls, 2.5, lam, period), locally_periodic_numpy(ls.numpy(), 2.5, lam.numpy(), period.numpy())
    a, b = kt(x1, x2).numpy(), kn(x1.numpy(), x2.numpy())
    assert np.abs(a - b).max() <= 16 * T.EPS * 2.5  # (the exponent is O(1) here: a few eps from each sine library)
    assert np.all(kt(x1, x1).diagonal().numpy() == 2.5) and np.all(np.diag(kn(x1.numpy(), x1.numpy())) == 2.5)
    far = torch.full((1, 3), float("inf"), dtype=F64)
    assert torch.isnan(kt(far, -far)).all() and np.isnan(kn(far.numpy(), -far.numpy())).all(), "a non-finite difference: NaN"
    # the product of the two factors it is made of
    from periodic_closed_form import periodic_torch
    rbf = torch.exp(-0.5 * ((x1[:, None, :] - x2[None, :, :]) / ls).square().sum(-1))
    assert np.abs(a - (rbf * periodic_torch(lam, 2.5, period)(x1, x2)).numpy()).max() <= 16 * T.EPS * 2.5


@pytest.mark.parametrize("name", list(T.CASES))
def test_lapack_helper_is_a_legitimate_yardstick(name):
    """locally_periodic_truth.mll_and_grad against the 50-digit truth, per output relative to its sum-of-magnitudes scale S.
    The GPU bar of test_gpu_locally_periodic is max(16 e_cpu, 64 eps); the helper's own error must be at most 1/16 of it.
    That alone holds by construction, so the helper is also held to what a backward-stable Cholesky evaluation can show:
    n cond(K_y) eps relative to S (Higham, Accuracy and Stability, thm. 10.4 with the growth factor n)."""
    x, y, ls, lam, period = T.case_inputs(name)
    n, d = x.shape
    out, mag, e_cpu = T.cpu_case(name)
    assert out.shape == mag.shape == (4 + 3 * d,) and np.all(mag > 0)
    gpu_bar = np.maximum(16.0 * e_cpu, 64.0 * T.EPS)
    kap = T.kappa(x, ls, lam, period)
    cond = torch.linalg.cond(T.OUTPUTSCALE * kap + T.NOISE * torch.eye(n, dtype=F64)).item()
    print(f"{name}: e_cpu max {e_cpu.max():.2e} = {e_cpu.max() / T.EPS:.1f} eps, cond(K_y) {cond:.1e}, per output " +
          " ".join(f"{v / T.EPS:.1f}" for v in e_cpu))
    assert np.all(e_cpu <= gpu_bar / 16.0) and np.all(e_cpu <= n * cond * T.EPS)
    assert (kap > 1e-3).double().mean().item() >= 0.5, "test construction: most entries must be of the size of s"


@pytest.mark.parametrize("d", [1, 2, 3, 5, 8, 13, 16])
def test_the_draws_keep_the_entries_of_the_size_of_s(d):
    """the draws of the GPU file (x ~ N(0, I), l = (1 + U) sqrt(d), lambda = (0.5 + U) d, p = 0.5 + 2.5 U): on (65, 515) most
    entries of the closed form stay above 1e-3 s, so its construction assert rests on the reference alone"""
    g = torch.Generator().manual_seed(2000 * d + 10)
    x1, x2 = torch.randn(65, d, generator=g, dtype=F64), torch.randn(515, d, generator=g, dtype=F64)
    ls, lam, period = T.draw_parameters(g, d)
    kap = locally_periodic_factors_numpy(x1.numpy()[:, None, :] - x2.numpy()[None, :, :], ls.numpy(), lam.numpy(), period.numpy())[0]
    share = float((kap > 1e-3).mean())
    print(f"d={d}: {share:.3f} of the entries above 1e-3, largest exponent {-np.log(kap.min()):.1f}")
    assert share >= 0.5


# ---- kernel objects ------------------------------------------------------------------------------------------------------
def _stub(**attributes):
    return type("Stub", (), attributes)()


def _product_stub(members, outputscale):
    return _stub(base_kernel=_stub(kernels=members), outputscale=outputscale)


def test_kernel_class_and_validation():
    k = LocallyPeriodicKernel([0.5, 2.0, 1.25], 3.0, periodic_lengthscale=[0.9, 1.1, 0.6], period_length=[1.0, 0.7, 2.5])
    assert k.kind == L.KERNEL_LOCALLY_PERIODIC == T.LOCALLY_PERIODIC == 10 and k.outputscale == 3.0 and k.family == "locally_periodic"
    assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.periodic_lengthscale.tolist() == [0.9, 1.1, 0.6]
    assert k.period_length.tolist() == [1.0, 0.7, 2.5]
    assert k._lengthscale_host(3).tolist() == [0.5, 2.0, 1.25, 0.9, 1.1, 0.6, 1.0, 0.7, 2.5], "l, then lambda, then p"
    shared = LocallyPeriodicKernel([0.75], 1.5, periodic_lengthscale=0.5, period_length=2.0)
    assert shared._lengthscale_host(4).tolist() == [0.75] * 4 + [0.5] * 4 + [2.0] * 4, "a shared value is repeated per block"
    assert LocallyPeriodicKernel([1.0, 2.0], period_length=0.5)._lengthscale_host(2).tolist() == [1.0, 2.0, 1.0, 1.0, 0.5, 0.5]
    default = LocallyPeriodicKernel([1.0])
    assert default.periodic_lengthscale.tolist() == [1.0] and default.period_length.tolist() == [1.0] and default.outputscale == 1.0
    assert pkg.LocallyPeriodicKernel is LocallyPeriodicKernel and "LocallyPeriodicKernel" in pkg.__all__
    from projected_langevin_sampling_amd.kernel import STATIONARY_KERNELS, _StationaryKernel
    assert isinstance(k, _StationaryKernel) and LocallyPeriodicKernel in STATIONARY_KERNELS
    assert LocallyPeriodicKernel.shape_blocks == (("periodic_lengthscale", True), ("period_length", True))
    assert PeriodicKernel.shape_blocks == (("period_length", True),) and pkg.RQKernel.shape_blocks == (("alpha", False),)
    assert ARDKernel.shape_blocks == () and pkg.MaternKernel.shape_blocks == ()
    for bad in (0.0, -1.0, [1.0, 0.0], float("nan")):
        with pytest.raises(ValueError, match="period length"):
            LocallyPeriodicKernel([1.0, 1.0], 1.0, period_length=bad)
        with pytest.raises(ValueError, match="periodic lengthscale"):
            LocallyPeriodicKernel([1.0, 1.0], 1.0, periodic_lengthscale=bad)
        with pytest.raises(ValueError, match="every lengthscale"):
            LocallyPeriodicKernel(bad, 1.0)
    with pytest.raises(AssertionError, match="has 3 entries, data has 2 dims"):
        k._lengthscale_host(2)


def test_as_base_kernel_reads_a_scaled_product():
    rbf = _stub(lengthscale=torch.tensor([[0.5, 2.0, 1.25]]))
    periodic = _stub(lengthscale=torch.tensor([[0.875, 1.125, 0.625]]), period_length=torch.tensor([[1.0, 0.75, 2.5]]))  # (float32-exact)
    for members in ([rbf, periodic], (periodic, rbf)):  # either order: the member with a period length is the periodic one
        k = as_base_kernel(_product_stub(members, torch.tensor(3.0)))
        assert type(k) is LocallyPeriodicKernel and k.outputscale == 3.0
        assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.periodic_lengthscale.tolist() == [0.875, 1.125, 0.625]
        assert k.period_length.tolist() == [1.0, 0.75, 2.5]
    k = as_base_kernel(_product_stub([_stub(lengthscale=torch.tensor([[0.75]])),
                                      _stub(lengthscale=torch.tensor([[0.5]]), period_length=torch.tensor([[2.0]]))], 1.5))
    assert type(k) is LocallyPeriodicKernel and k._lengthscale_host(2).tolist() == [0.75, 0.75, 0.5, 0.5, 2.0, 2.0]
    assert as_base_kernel(k) is k
    # any other product is refused with the existing TypeError
    for members in ([rbf, rbf], [periodic, periodic], [rbf], [rbf, periodic, rbf], [rbf, _stub(period_length=torch.tensor([1.0]))],
                    [_stub(lengthscale=None), periodic], [_stub(lengthscale=torch.tensor([[1.0]]), nu=2.5), periodic]):
        with pytest.raises(TypeError, match="unsupported base kernel"):
            as_base_kernel(_product_stub(members, 1.0))
    # the single-kernel readings are as they were
    plain = _stub(base_kernel=_stub(lengthscale=torch.tensor([[1.0]]), period_length=torch.tensor([[2.0]])), outputscale=1.0)
    assert type(as_base_kernel(plain)) is PeriodicKernel
    assert type(as_base_kernel(_stub(base_kernel=_stub(lengthscale=torch.tensor([[1.0]])), outputscale=1.0))) is ARDKernel


# ---- the raw layout ------------------------------------------------------------------------------------------------------
def _data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    return x, torch.sin(x.sum(dim=1)) + 0.1 * torch.randn(n, generator=g, dtype=F64)


def test_exact_gp_raw_layout_and_start_values():
    x, y = _data(12, 3, 1)
    model = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel)
    assert model.kind == L.KERNEL_LOCALLY_PERIODIC and model.kernel_name == "locally_periodic" and model.raw.shape == (12,)  # 3 + 3 nls
    assert torch.equal(model.raw.detach(), torch.zeros(12, dtype=F64))
    for values in (model.lengthscale, model.periodic_lengthscale, model.period_length):
        assert values.shape == (3,) and torch.allclose(values, torch.full((3,), LN2, dtype=F64), rtol=1e-15)
    assert not hasattr(model, "alpha") and not hasattr(pkg.ExactGP(x, y, kernel="rbf"), "periodic_lengthscale")
    assert not hasattr(pkg.ExactGP(x, y, kernel=PeriodicKernel), "periodic_lengthscale")
    assert pkg.ExactGP(x, y, kernel=PeriodicKernel).period_length.shape == (3,)
    shared = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel, ard=False)
    assert shared.raw.shape == (6,) and shared.period_length.shape == (3,) and shared.periodic_lengthscale.shape == (3,)
    assert shared._library_lengthscale().shape == (1, 9)
    start = LocallyPeriodicKernel([0.5, 2.0, 1.25], 1.7, periodic_lengthscale=[0.9, 1.1, 0.6], period_length=[1.0, 0.7, 2.5])
    model = pkg.ExactGP(x, y, kernel=start)
    assert model.kind == L.KERNEL_LOCALLY_PERIODIC and model.ard and model.raw.shape == (12,)
    # the round trip start kernel -> raw -> library values
    assert torch.allclose(model._library_lengthscale()[0], start._lengthscale_host(3), rtol=1e-14)
    assert torch.allclose(model.periodic_lengthscale, start.periodic_lengthscale, rtol=1e-14)
    assert torch.allclose(model.period_length, start.period_length, rtol=1e-14) and model.outputscale == pytest.approx(1.7, rel=1e-14)
    fitted = model.kernel
    assert type(fitted) is LocallyPeriodicKernel and fitted.outputscale == model.outputscale
    assert torch.equal(fitted.lengthscale, model.lengthscale) and torch.equal(fitted.period_length, model.period_length)
    assert torch.equal(fitted.periodic_lengthscale, model.periodic_lengthscale)
    assert torch.equal(fitted._lengthscale_host(3), model._library_lengthscale()[0])
    one = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel([0.8], 1.1, periodic_lengthscale=[0.6], period_length=[1.3]))
    assert not one.ard and one.raw.shape == (6,)
    assert torch.allclose(one._library_lengthscale()[0], torch.tensor([0.8] * 3 + [0.6] * 3 + [1.3] * 3, dtype=F64), rtol=1e-14)
    for mixed in (LocallyPeriodicKernel([0.8], 1.1, period_length=[1.0, 0.7, 2.5]),
                  LocallyPeriodicKernel([0.8], 1.1, periodic_lengthscale=[1.0, 0.7, 2.5])):  # a per-dimension block: ard
        model2 = pkg.ExactGP(x, y, kernel=mixed)
        assert model2.ard and model2.raw.shape == (12,) and torch.allclose(model2.lengthscale, torch.full((3,), 0.8, dtype=F64), rtol=1e-14)
        assert torch.allclose(model2._library_lengthscale()[0], mixed._lengthscale_host(3), rtol=1e-14)
    # the raw order: lengthscales, periodic lengthscales, period lengths
    raw = torch.tensor([0.1, -1.0, 0.3, 0.2, 0.6, -0.4, 1.5, -0.7, 0.9, -0.3, 0.8, 0.05], dtype=F64)
    assert torch.equal(model.set_raw_parameters(raw).raw_parameters(), raw)
    assert torch.allclose(model.lengthscale, sp(raw[3:6]), rtol=1e-15) and torch.allclose(model.periodic_lengthscale, sp(raw[6:9]), rtol=1e-15)
    assert torch.allclose(model.period_length, sp(raw[9:12]), rtol=1e-15)
    lib = model._library_lengthscale()
    assert lib.shape == (1, 9) and torch.equal(lib[0, :3], model.lengthscale) and torch.equal(lib[0, 3:6], model.periodic_lengthscale)
    assert torch.equal(lib[0, 6:], model.period_length)
    with pytest.raises(AssertionError):
        model.set_raw_parameters(raw[:11])


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_widths_follow_the_library_count(ard):
    """the width checks of test_kernel_family_host.py for the family with two blocks: _lengthscale_host, _library_lengthscale,
    the raw width and the chain_rule shape, tied to the library's own count through the workspace query"""
    d = 3
    lib = L.load()
    for n, dd in ((515, 5), (130, 16)):
        blocks = -(-n // 512) * -(-n // 64)
        assert lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_LOCALLY_PERIODIC, n, dd) == 8 * blocks * (3 * dd + 1)
        assert L.kernel_shape_params(L.KERNEL_LOCALLY_PERIODIC, dd) == 2 * dd
    x, y = _data(10, d, 3)
    keywords = ({"periodic_lengthscale": [0.9, 1.1, 0.6], "period_length": [1.5, 0.5, 2.0]} if ard
                else {"periodic_lengthscale": 0.9, "period_length": 1.5})
    kernel = LocallyPeriodicKernel([0.5, 1.0, 2.0] if ard else [0.5], 1.3, **keywords)
    assert kernel._lengthscale_host(d).numel() == 3 * d
    model = pkg.ExactGP(x, y, kernel=kernel, ard=ard)
    nls = d if ard else 1
    assert model.raw.numel() == 3 + 3 * nls == 3 + nls + L.kernel_shape_params(model.kind, nls)
    assert model._library_lengthscale().shape == (1, 3 * d)
    assert torch.allclose(model._library_lengthscale()[0], kernel._lengthscale_host(d), rtol=1e-14)
    loss, grad = model.chain_rule(torch.arange(4 + 3 * d, dtype=F64))
    assert grad.shape == model.raw.shape and loss == 0.0
    assert type(model.kernel) is LocallyPeriodicKernel and model.kernel._lengthscale_host(d).numel() == 3 * d


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_sums_block_by_block(ard):
    """chain_rule fed an ``out`` whose entries are known: out[4 + j] = (j + 1) v_j with v the library's natural values, so that
    d/d natural value j is j + 1.  Per dimension, raw column c of a block gets (j + 1) sigmoid(raw); a shared raw column gets
    the sum of ITS OWN block's d entries, (sum of j + 1 over the block) sigmoid(raw), and nothing of its neighbours'."""
    d, n = 3, 10
    x, y = _data(n, d, 4)
    model = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel, ard=ard)
    nls = d if ard else 1
    raw = 0.5 * torch.randn(3 + 3 * nls, generator=torch.Generator().manual_seed(5), dtype=F64)
    model.set_raw_parameters(raw)
    natural = model._library_lengthscale()[0]
    out = torch.zeros(4 + 3 * d, dtype=F64)
    out[4:] = torch.arange(1, 3 * d + 1, dtype=F64) * natural
    _, grad = model.chain_rule(out)
    slope = torch.sigmoid(raw)
    for block in range(3):
        weights = torch.arange(1 + block * d, 1 + (block + 1) * d, dtype=F64)
        columns = slice(3 + block * nls, 3 + (block + 1) * nls)
        want = (weights if ard else weights.sum(dim=0, keepdim=True)) * slope[columns]
        assert torch.allclose(grad[columns], -want / n, rtol=1e-14), (block, grad[columns], -want / n)
    assert torch.equal(grad[:3], torch.zeros(3, dtype=F64))


def test_dirichlet_raw_layout():
    x, _ = _data(12, 2, 2)
    labels = torch.arange(12) % 3
    model = pkg.DirichletExactGP(x, labels, kernel=LocallyPeriodicKernel)
    assert model.kind == L.KERNEL_LOCALLY_PERIODIC and model.raw.shape == (3, 9) and model.period_length.shape == (3, 2)
    assert model.periodic_lengthscale.shape == (3, 2)
    raw = 0.3 * torch.randn(3, 9, generator=torch.Generator().manual_seed(4), dtype=F64)
    model.set_raw_parameters(raw)
    assert torch.equal(model.raw_parameters(), raw)
    assert torch.allclose(model.lengthscale, sp(raw[:, 3:5]), rtol=1e-15) and torch.allclose(model.periodic_lengthscale, sp(raw[:, 5:7]), rtol=1e-15)
    assert torch.allclose(model.period_length, sp(raw[:, 7:9]), rtol=1e-15)
    ls = model._library_lengthscale()
    assert ls.shape == (3, 6) and torch.equal(ls[:, :2], model.lengthscale) and torch.equal(ls[:, 2:4], model.periodic_lengthscale)
    assert torch.equal(ls[:, 4:], model.period_length)
    kernels = model.kernels
    assert [type(k) for k in kernels] == [LocallyPeriodicKernel] * 3
    assert all(torch.equal(k._lengthscale_host(2), ls[c]) for c, k in enumerate(kernels))
    one = model.kernel  # the raw values averaged over the classes, softplus afterwards
    assert type(one) is LocallyPeriodicKernel and torch.allclose(one.period_length, sp(raw[:, 7:9].mean(dim=0)), rtol=1e-15)
    assert torch.allclose(one.periodic_lengthscale, sp(raw[:, 5:7].mean(dim=0)), rtol=1e-15)
    assert pkg.DirichletExactGP(x, labels, kernel=LocallyPeriodicKernel, ard=False).raw.shape == (3, 6)


def test_the_names_the_model_classes_and_the_trainers_take():
    x, y = _data(12, 3, 5)
    with pytest.raises(ValueError, match="kernel must be one of"):  # (the model classes take the class; the trainers the name)
        pkg.ExactGP(x, y, kernel="locally_periodic")
    with pytest.raises(TypeError, match="PeriodicKernel"):
        pkg.ExactGP(x, y, kernel=pkg.LinearKernel())


# ---- chain_rule against central differences ----------------------------------------------------------------------------
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
def test_chain_rule_against_central_differences(ard):
    """chain_rule fed with the LAPACK helper's 4 + 3 d outputs against central differences of the helper's own value in every
    raw parameter, step h = 1e-5, with the periodic host test's bar (1e-7 of the largest gradient component: truncation
    h^2 |f'''| / 6 and rounding eps |f| / h are both 2e-11 of |f'''| and |f|)."""
    x, y = _data(40, 3, 6)
    model = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel, ard=ard)
    g = torch.Generator().manual_seed(7 + ard)
    raw = 0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64)
    raw[1] = -2.0  # noise = 1e-4 + softplus(-2) = 0.127
    model.set_raw_parameters(raw)
    out, _ = T.mll_and_grad(x, y, model.lengthscale, model.periodic_lengthscale, model.period_length, model.outputscale, model.noise,
                            model.mean_constant)
    assert out.shape == (4 + 9,)
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
    print(f"{'ard' if ard else 'shared'}: gradient rel err {err:.2e}; d/d raw shape blocks {grad[3:].tolist()}")
    assert err <= 1e-7
    assert grad[3:].abs().min() > 1e-4 * want.abs().max(), "test construction: every block's derivatives must matter"


def test_construct_average_ard_kernel_on_two_models():
    x, y = _data(12, 2, 8)
    a, b = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel), pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel)
    a.set_raw_parameters(torch.tensor([0.0, 0.0, 0.2, 0.4, -0.6, 1.0, 0.5, 0.25, -1.0], dtype=F64))
    b.set_raw_parameters(torch.tensor([0.5, 0.1, 0.6, -0.2, 0.2, -2.0, 0.25, 0.75, 2.0], dtype=F64))
    k = pkg.construct_average_ard_kernel([a, b])
    assert type(k) is LocallyPeriodicKernel and k.outputscale == float(sp(torch.tensor(0.4, dtype=F64)))
    assert torch.equal(k.lengthscale, sp(torch.tensor([0.1, -0.2], dtype=F64)))
    assert torch.equal(k.periodic_lengthscale, sp(torch.tensor([-0.5, 0.375], dtype=F64))), "every block is averaged"
    assert torch.equal(k.period_length, sp(torch.tensor([0.5, 0.5], dtype=F64)))
    shared = pkg.ExactGP(x, y, kernel=LocallyPeriodicKernel, ard=False)
    k = pkg.construct_average_ard_kernel([shared])
    assert type(k) is LocallyPeriodicKernel and k.lengthscale.numel() == 2 and k.period_length.numel() == 2
    assert k.periodic_lengthscale.numel() == 2 and torch.allclose(k.period_length, torch.full((2,), LN2, dtype=F64), rtol=1e-15)


def test_training_loop_and_runner_accept_the_name():
    """train_exact_gp with kernel="locally_periodic", with the class and with an instance, on the host evaluation"""
    x, y = _data(30, 2, 9)
    args = dict(seed=1, learning_rate=0.05, early_stopper_patience=10.0)
    model, losses = pkg.train_exact_gp(x, y, "locally_periodic", number_of_epochs=5, evaluate=T.host_evaluate, **args)
    assert model.kind == L.KERNEL_LOCALLY_PERIODIC and len(losses) == 5 and losses[-1] < losses[0]
    assert torch.all(model.raw_parameters()[3:] != 0.0), "all three blocks are learned"
    by_class, losses2 = pkg.train_exact_gp(x, y, LocallyPeriodicKernel, number_of_epochs=5, evaluate=T.host_evaluate, **args)
    assert losses2 == losses and torch.equal(by_class.raw_parameters(), model.raw_parameters())
    start = LocallyPeriodicKernel([1.0, 2.0], 1.0, periodic_lengthscale=[0.7, 1.2], period_length=[1.3, 0.9])
    model, _ = pkg.train_exact_gp(x, y, start, number_of_epochs=1, evaluate=T.host_evaluate, **args)
    assert model.kind == L.KERNEL_LOCALLY_PERIODIC and model.raw.shape == (9,)
    model, _ = pkg.train_exact_gp(x, torch.arange(30) % 2, "locally_periodic", number_of_epochs=0, likelihood="dirichlet", **args)
    assert type(model) is pkg.DirichletExactGP and model.raw.shape == (2, 9)


# ---- the C ABI (validation only: no HIP call) ---------------------------------------------------------------------------
def test_cabi_accepts_the_kind_and_sizes_its_workspace():
    lib = L.load()
    p = 8  # (any non-NULL address: every call below fails its argument checks first)
    K = L.KERNEL_LOCALLY_PERIODIC
    assert lib.pls_abi_version() == L.ABI_VERSION == 7 and K == 10
    assert lib.pls_kernel_gram(K, p, 1, p, 1, 1, None, 1.0, p, 1, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(K, p, 4, 1, None, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
    assert b"lengthscale" in lib.pls_last_error() and b"unknown" not in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, None, 1.0, 0.0, p, p, 3, p, None) == 1 and b"NULL pointer" in lib.pls_last_error()
    assert lib.pls_kernel_mean(K, p, 4, 2, p, 1.0, 0.0, p, p, 0, p, None) == 0
    # 3 d + 1 sums and 4 + 3 d outputs
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5) == 8 * 16 * 2 * 9
    assert lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 130, 16) == 8 * 49 * 1 * 3
    assert lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3) > lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_PERIODIC, 5, 3)
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 2) == lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert lib.pls_gp_mll_classes_workspace_bytes_kind(K, 5, 3, 0) == 0
    # d = 17 is refused, by the queries with 0 and by every entry with the kind's own message
    msg = b"> 16 is not supported for the locally periodic kernel"
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
    # kind 9 is refused as unknown, like 5 and 7, by the entries that the other host tests probe with 5
    for bad in (9, 5, 7, 11, -1):
        unknown = f"unknown kernel kind {bad}".encode()
        assert lib.pls_gp_mll_workspace_bytes_kind(bad, 5, 3) == 0 and lib.pls_kernel_grad_sums_workspace_bytes_kind(bad, 5, 3) == 0
        assert lib.pls_gp_mll_classes_workspace_bytes_kind(bad, 5, 3, 2) == 0
        assert lib.pls_kernel_gram(bad, p, 1, p, 1, 1, p, 1.0, p, 1, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_kernel_mean(bad, p, 4, 2, p, 1.0, 0.0, p, p, 3, p, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_kernel_grad_sums(bad, p, 5, 3, p, 1.0, p, p, 5, p, 16, 1 << 20, None) == 1 and unknown in lib.pls_last_error()
        assert lib.pls_gp_mll_grad(bad, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, 1 << 20, None) == 1
        assert unknown in lib.pls_last_error()
        assert lib.pls_gp_mll_grad_classes(bad, p, 5, 3, 2, p, p, p, p, None, 5, p, 5, 0.0, p, p, 16, 1 << 20, None) == 1
        assert unknown in lib.pls_last_error()
        assert lib.pls_select_inducing_conditional_variance(bad, p, 4, 1, p, 1.0, 2, 1e-12, 0.0, p, p, None, 0, None) == 1
        assert unknown in lib.pls_last_error()
    # the entries check against the kind-aware need: the periodic size is too small for 3 d + 1 sums
    old, need = lib.pls_gp_mll_workspace_bytes_kind(L.KERNEL_PERIODIC, 5, 3), lib.pls_gp_mll_workspace_bytes_kind(K, 5, 3)
    assert lib.pls_gp_mll_grad(K, p, 5, 3, p, 1.0, 0.1, 0.0, 0.0, p, p, p, 16, old, None) == 3  # WORKSPACE_TOO_SMALL
    assert f"{need} needed".encode() in lib.pls_last_error()
    old, need = lib.pls_kernel_grad_sums_workspace_bytes_kind(L.KERNEL_PERIODIC, 515, 5), lib.pls_kernel_grad_sums_workspace_bytes_kind(K, 515, 5)
    assert lib.pls_kernel_grad_sums(K, p, 515, 5, p, 1.0, p, p, 515, p, 16, old, None) == 3
    assert f"{need} needed".encode() in lib.pls_last_error()
