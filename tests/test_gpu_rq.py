"""GPU: the rational-quadratic base kernel end to end -- the Gram build against the closed form (every D_MAX instantiation,
both store paths, small and large alpha) and its exact properties, the d + 2 sums of the gradient reduction per output,
the whole marginal-likelihood evaluation against 50-digit arithmetic (one class and the classes entry), the fused
predictive mean per test point, the conditional-variance selector, training against the same loop on the CPU, one ONB and
one IPB step per native cost against the CPU oracle on the closed form, and the hand-over of a learned kernel to PLS and
to the SVGP baseline."""
import ctypes
import math

import numpy as np
import pytest
import torch

import base_kernel_calls as C
import rq_truth as T
import svgp_truth as ST
from base_kernel_calls import gram_into as _gram_into, lib_params as lib_ls, offset_copy, p_views
from oracle import pls_oracle as O
from rq_closed_form import ALPHAS, LN2, rq_numpy, rq_torch
from test_gpu_parity import P, TOL, _f64_default, cu, make_costs, make_problem, relerr, step_tolerance  # noqa: F401

pytestmark = pytest.mark.gpu

F64 = torch.float64
DIMS = [1, 2, 3, 5, 8, 13, 33, 64]  # every D_MAX of the pairwise kernels: 1, 2, 4, 8, 16, 32, 64, padded and exact
ALPHA_IDS = [f"alpha={a:g}" for a in ALPHAS]
RQ = T.RQ
note = C.make_note()


def draw(g, n, d):
    """x ~ N(0, 1), lengthscales (0.5 - 1.5) sqrt(d), as the existing tests draw their problems"""
    return torch.randn(n, d, generator=g, dtype=F64), (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5


# ---- 1. the Gram build ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS, ids=ALPHA_IDS)
@pytest.mark.parametrize("d", DIMS)
def test_gram_against_the_closed_form(P, d, alpha):
    """(65, 515): a second row block of one row, a second column block with an odd tail; (1, 1).  Per entry within 1e-13 s of
    the closed form and norm-wise relerr < 1e-13; the scalar store path (odd ldout, 8 bytes off) gives the same bits."""
    g = torch.Generator().manual_seed(2000 * d + int(alpha * 7) % 997)
    s = 2.5
    for n1, n2 in ((65, 515), (1, 1)):
        (x1, ls), x2 = draw(g, n1, d), torch.randn(n2, d, generator=g, dtype=F64)
        k = P.pkg.RQKernel(ls, s, alpha=alpha)
        want = rq_torch(ls, s, alpha)(x1, x2)
        got = k(x1, x2)
        assert not torch.isnan(got).any()
        entry = ((got.cpu() - want).abs().max() / (1e-13 * s)).item()
        norm = relerr(got, want) / 1e-13
        note("gram", f"d={d} alpha={alpha:g} ({n1}, {n2}) per entry", entry)
        note("gram", f"d={d} alpha={alpha:g} ({n1}, {n2}) norm-wise", norm)
        assert entry <= 1.0 and norm < 1.0
        ldout = n2 + 2
        buf = torch.full((1 + n1 * ldout,), float("nan"), dtype=F64, device="cuda")
        view = buf[1:].view(n1, ldout)
        assert view.data_ptr() % 16 == 8 and ldout % 2 == 1
        _gram_into(P, k, x1, x2, view, ldout)
        assert torch.equal(view[:, :n2], got), "scalar store path != 16-byte store path"
        assert torch.isnan(view[:, n2:]).all() and torch.isnan(buf[:1]).all()
        if n1 > 1:
            assert (want > 1e-3 * s).double().mean().item() >= 0.5, "test construction: most entries must be of the size of s"


@pytest.mark.parametrize("alpha", ALPHAS, ids=ALPHA_IDS)
def test_gram_exact_properties(P, alpha):
    g = torch.Generator().manual_seed(5)
    d, s = 5, 1.7
    z = torch.randn(131, d, generator=g, dtype=F64)
    ls = 0.5 + torch.rand(d, generator=g, dtype=F64)
    k = P.pkg.RQKernel(ls, s, alpha=alpha)
    kzz = k(z, z)
    assert torch.equal(kzz, kzz.T), "k(Z, Z) is not exactly symmetric"
    assert torch.all(kzz.diagonal() == s), "k(x, x) is not the outputscale to the bit"
    pick = torch.randperm(131, generator=g)[:77]
    x2 = torch.cat([torch.randn(40, d, generator=g, dtype=F64), z[pick]])
    kx = k(z, x2).cpu()
    assert torch.all(kx[pick, 40 + torch.arange(77)] == s)
    # r = inf: exactly 0, no NaN, whatever alpha
    far = torch.cat([torch.full((3, d), 1e200, dtype=F64), torch.full((2, d), -1e200, dtype=F64)])
    kf = k(far, -far).cpu()
    assert not torch.isnan(kf).any()
    assert torch.all(kf[:3, :3] == 0) and torch.all(kf[3:, 3:] == 0)
    assert torch.all(k(far, torch.zeros(4, d, dtype=F64)).cpu() == 0)


def test_a_far_point_dies_only_for_a_large_alpha(P):
    """A point 1e4 lengthscales away: exactly 0 at alpha = 1e3 (alpha log1p(u) = 1.08e4 > 745.2), the truth -- 3.3e-6, not
    0 -- at alpha = ln 2, held to the Gram bar."""
    g = torch.Generator().manual_seed(6)
    d, s = 3, 1.7
    x, ls = draw(g, 4, d)
    far = x[:1] + 1e4 * ls / math.sqrt(d) * torch.ones(1, d, dtype=F64)  # r = 1e4 exactly up to rounding
    assert torch.all(P.pkg.RQKernel(ls, s, alpha=1e3)(far, x[:1]).cpu() == 0.0)
    got = P.pkg.RQKernel(ls, s, alpha=LN2)(far, x).cpu()
    want = rq_torch(ls, s, LN2)(far, x)
    assert 1e-6 * s < want[0, 0].item() < 1e-5 * s, "test construction"
    err = (got - want).abs().max().item()
    note("far point", "alpha=ln2", err / (1e-13 * s))
    assert err <= 1e-13 * s and torch.all(got > 0) and relerr(got, want) < 1e-13


# ---- 2. the reduction ----------------------------------------------------------------------------------------------------
def grad_sums(P, x, ls, shape, s, alpha, p_view, ldp):
    """pls_kernel_grad_sums for PLS_KERNEL_RQ: the d + 2 sums"""
    return C.grad_sums(P, RQ, x, lib_ls(ls, shape), s, alpha, p_view, ldp)


def reduction_problem(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x, ls = draw(g, n, d)
    alpha = torch.randn(n, generator=g, dtype=F64)
    a = torch.randn(n, n, generator=g, dtype=F64)
    return x, ls, alpha, a + a.T


def check_sums(tag, got, want, scale):
    """the bar of test_gpu_exact_gp.test_reduction_per_output: |got - want| <= 1e-13 * sum|term| per output"""
    ratio = np.abs(got.numpy() - want) / np.where(scale > 0, 1e-13 * scale, 1.0)
    note("reduction", tag + f" (alpha sum {ratio[-1]:.2e})", ratio.max())
    assert np.all(np.isfinite(got.numpy())), (tag, got)
    assert np.all(np.abs(got.numpy() - want) <= 1e-13 * scale), (tag, ratio)


@pytest.mark.parametrize("n,d,alpha", [(515, 5, LN2), (515, 5, 1e3)] + [(130, d, ALPHAS[i % len(ALPHAS)]) for i, d in enumerate(DIMS)])
def test_reduction_per_output(P, n, d, alpha):
    s = 1.7
    x, ls, al, p = reduction_problem(n, d, 7000 + 10 * n + d)
    want, scale = T.grad_sums(x, ls, alpha, s, al, p)
    assert want.shape == (d + 2,) and scale[-1] > 0
    (buf, ldp), (view, ldo) = p_views(p)
    got = grad_sums(P, x, ls, alpha, s, al, buf, ldp)
    check_sums(f"n={n} d={d} alpha={alpha:g}", got, want, scale)
    assert torch.equal(got, grad_sums(P, x, ls, alpha, s, al, buf, ldp)), "two calls differ"
    assert torch.equal(got, grad_sums(P, x, ls, alpha, s, al, view, ldo)), "scalar load path != 16-byte load path"


@pytest.mark.parametrize("alpha", [LN2, 1e3], ids=["alpha=ln2", "alpha=1e3"])
def test_reduction_with_a_duplicated_point(P, alpha):
    """Pairs at distance 0 (across column pairs and row blocks) contribute 0 to every lengthscale sum and exactly 0 to the
    alpha sum: with every point equal, those sums are exactly 0 and the first is sum W."""
    n, d, s = 130, 5, 1.7
    x, ls, al, p = reduction_problem(n, d, 8100)
    x[10], x[11], x[70], x[129] = x[3], x[3], x[3], x[64]
    (buf, ldp), _ = p_views(p)
    want, scale = T.grad_sums(x, ls, alpha, s, al, p)
    check_sums(f"duplicates alpha={alpha:g}", grad_sums(P, x, ls, alpha, s, al, buf, ldp), want, scale)
    same = x[3:4].expand(n, d).contiguous()
    got = grad_sums(P, same, ls, alpha, s, al, buf, ldp)
    assert torch.all(got[1:] == 0.0), got
    w = al[:, None] * al[None, :] - p
    assert abs(got[0].item() - math.fsum(w.reshape(-1).tolist())) <= 1e-13 * w.abs().sum().item()
    x[5], x[6], x[100] = 1e200, 1e200, -1e200  # r = inf: no contribution, nothing becomes NaN
    want, scale = T.grad_sums(x, ls, alpha, s, al, p)
    assert np.all(np.isfinite(want))
    check_sums(f"far points alpha={alpha:g}", grad_sums(P, x, ls, alpha, s, al, buf, ldp), want, scale)


# ---- 3. the whole evaluation -------------------------------------------------------------------------------------------
def gp_mll(P, x, y, ls, shape, s, noise, mean, jitter=0.0, fill=None):
    """pls_gp_mll_grad for PLS_KERNEL_RQ: (the 5 + d outputs on the CPU, info, status)"""
    return C.gp_mll(P, RQ, x, y, lib_ls(ls, shape), s, noise, mean, jitter, fill)


@pytest.mark.parametrize("name", list(T.CASES))
def test_whole_evaluation_against_50_digits(P, name):
    """Every output against the 50-digit truth, relative to its sum-of-magnitudes scale S.  Bar per output:
    max(16 e_cpu, 64 eps), exactly as test_gpu_exact_gp.test_whole_evaluation_against_50_digits."""
    x, y, ls, shape = T.case_inputs(name)
    _, mag, e_cpu = T.cpu_case(name)
    hi, lo = T.truth(name)
    got, info, rc = gp_mll(P, x, y, ls, shape, T.OUTPUTSCALE, T.NOISE, T.MEAN)
    assert rc == 0 and info == 0
    err = T.relative_error(got.numpy(), hi, lo, mag)
    bar = np.maximum(16.0 * e_cpu, 64.0 * T.EPS)
    print(f"{name}: max err/S {err.max():.2e}  (e_cpu max {e_cpu.max():.2e})  per output err/bar " + " ".join(f"{v:.3f}" for v in err / bar))
    note("whole evaluation", name, np.max(err / bar))
    again, _, _ = gp_mll(P, x, y, ls, shape, T.OUTPUTSCALE, T.NOISE, T.MEAN)
    assert torch.equal(got, again), "two calls differ"
    poisoned, info, rc = gp_mll(P, x, y, ls, shape, T.OUTPUTSCALE, T.NOISE, T.MEAN, fill=float("nan"))
    assert rc == 0 and info == 0 and torch.equal(got, poisoned), "the result depends on what the workspace held"
    assert np.all(err <= bar), (name, err / bar)


def test_classes_entry_equals_the_one_class_calls(P):
    """pls_gp_mll_grad_classes with C = 2 (rows of d + 1 lengthscale values, rows of 5 + d outputs) and a fixed-noise vector:
    without the vector row c is pls_gp_mll_grad bit for bit; with it, it is the one-class call of the classes entry and
    agrees with the LAPACK helper."""
    L = P.pkg._lib
    lib = L.load()
    x, y, ls, shape = T.case_inputs("rq-n65-d3-aln2")
    n, d = x.shape
    g = torch.Generator().manual_seed(31)
    ls2, shape2 = ls * 1.3, 2.5
    ys = torch.stack([y, y.flip(0)])
    fixed = 0.05 + 0.1 * torch.rand(2, n, generator=g, dtype=F64)
    s, noise, mean = [T.OUTPUTSCALE, 0.9], [T.NOISE, 0.2], [T.MEAN, -0.1]
    lsd = torch.stack([torch.cat([ls, torch.tensor([shape], dtype=F64)]), torch.cat([ls2, torch.tensor([shape2], dtype=F64)])]).cuda().contiguous()
    xd, yd, fd = cu(x).contiguous(), cu(ys).contiguous(), cu(fixed).contiguous()
    nbytes = lib.pls_gp_mll_classes_workspace_bytes_kind(RQ, n, d, 2)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    host = ctypes.c_double * 2

    def classes(c0, count, fixed_dev):
        out = torch.full((count * (5 + d) + 1,), float("nan"), dtype=F64, device="cuda")
        info = torch.full((count,), -7, dtype=torch.int32, device="cuda")
        hs, hn, hm = host(*s[c0:] + [0.0] * c0), host(*noise[c0:] + [0.0] * c0), host(*mean[c0:] + [0.0] * c0)
        rc = lib.pls_gp_mll_grad_classes(RQ, xd.data_ptr(), n, d, count, lsd[c0:].data_ptr(), ctypes.cast(hs, ctypes.c_void_p),
                                         ctypes.cast(hn, ctypes.c_void_p), ctypes.cast(hm, ctypes.c_void_p),
                                         fixed_dev[c0:].data_ptr() if fixed_dev is not None else None, n, yd[c0:].data_ptr(), n, 0.0,
                                         out.data_ptr(), info.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr())
        assert rc == 0 and not info.cpu().any() and torch.isnan(out[-1]).item()
        return out[:-1].cpu().reshape(count, 5 + d)

    both = classes(0, 2, None)
    for c, (lc, sc) in enumerate(((ls, shape), (ls2, shape2))):
        one, info, rc = gp_mll(P, x, ys[c], lc, sc, s[c], noise[c], mean[c])
        assert rc == 0 and info == 0 and torch.equal(both[c], one), f"class {c} != pls_gp_mll_grad"
    both = classes(0, 2, fd)
    assert torch.equal(both[0:1], classes(0, 1, fd)) and torch.equal(both[1:2], classes(1, 1, fd))
    for c, (lc, sc) in enumerate(((ls, shape), (ls2, shape2))):
        want, mag = T.mll_and_grad(x, ys[c], lc, sc, s[c], noise[c], mean[c], fixed=fixed[c])
        assert np.all(np.abs(both[c].numpy() - want) <= 1e-12 * mag), c


def test_not_positive_definite_is_reported_not_thrown(P):
    """noise = 0, jitter = 0 and two identical rows: the second pivot is exactly 0 (kappa = 1 exactly, outputscale 1)"""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(70, 3, generator=g, dtype=F64)
    x[1] = x[0]
    y = torch.randn(70, generator=g, dtype=F64)
    _, info, rc = gp_mll(P, x, y, torch.full((3,), 1.2, dtype=F64), 1.5, 1.0, 0.0, 0.0)
    assert rc == 0 and info == 2, (rc, info)
    loss, grad = P.pkg.ExactGP(x, y, "rq").loss_and_grad()
    assert np.isfinite(loss) and torch.isfinite(grad).all() and grad.shape == (7,)


def test_model_evaluation_is_gp_mll_grad(P):
    x, y, _, _ = T.case_inputs("rq-n65-d3-aln2")
    for ard in (True, False):
        model = P.pkg.ExactGP(x, y, "rq", ard=ard)
        g = torch.Generator().manual_seed(900 + ard)
        model.set_raw_parameters(0.5 * torch.randn(model.raw.numel(), generator=g, dtype=F64))
        out, info = model.evaluate_on_device(0.0)
        want, flag, rc = gp_mll(P, x, y, model.lengthscale, model.alpha, model.outputscale, model.noise, model.mean_constant)
        assert rc == 0 and flag == 0 and info == 0 and out.shape == (8,) and torch.equal(out, want), ard


# ---- 4. the fused predictive mean ----------------------------------------------------------------------------------------
S_MEAN, MEAN = 1.7, 0.3


def kernel_mean(P, xd, lsd, ad, xtd, s=S_MEAN, mean=MEAN):
    return C.kernel_mean(P, RQ, xd, lsd, ad, xtd, s, mean)


def mean_truth(x, ls, shape, s, mean, alpha, xt):
    """per test point: the exactly rounded sum of mean and the terms s kappa_ij alpha_j, and S_i = |mean| + s sum_j |kappa_ij alpha_j|"""
    terms = (rq_torch(ls, s, shape)(xt, x) * alpha[None, :]).numpy()
    want = np.array([math.fsum([float(mean)] + row.tolist()) for row in terms])
    return want, np.array([abs(float(mean)) + math.fsum(np.abs(row).tolist()) for row in terms])


def mean_problem(n, t, d, seed):
    g = torch.Generator().manual_seed(seed)
    x, ls = draw(g, n, d)
    return x, ls, torch.randn(n, generator=g, dtype=F64), torch.randn(t, d, generator=g, dtype=F64)


def check_mean(tag, got, want, scale):
    ratio = np.abs(got.numpy() - want) / (1e-13 * scale)
    note("mean", tag, ratio.max())
    assert np.all(np.isfinite(got.numpy())) and np.all(np.abs(got.numpy() - want) <= 1e-13 * scale), (tag, ratio.max())


MEAN_SIZES = [(n, t, 5) for n in (1, 2, 65, 515) for t in (1, 2, 65, 130)] + [(130, 70, d) for d in DIMS]


@pytest.mark.parametrize("k,n,t,d", [(i % len(ALPHAS), n, t, d) for i, (n, t, d) in enumerate(MEAN_SIZES)])
def test_mean_per_point(P, k, n, t, d):
    alpha = ALPHAS[k]
    x, ls, al, xt = mean_problem(n, t, d, 9000 + 100 * n + 10 * t + d)
    want, scale = mean_truth(x, ls, alpha, S_MEAN, MEAN, al, xt)
    xd, lsd, ad, xtd = cu(x).contiguous(), lib_ls(ls, alpha), cu(al).contiguous(), cu(xt).contiguous()
    assert xd.data_ptr() % 16 == 0 and xtd.data_ptr() % 16 == 0
    got = kernel_mean(P, xd, lsd, ad, xtd)
    check_mean(f"n={n} t={t} d={d} alpha={alpha:g}", got, want, scale)
    assert torch.equal(got, kernel_mean(P, xd, lsd, ad, xtd)), "two calls differ"
    assert torch.equal(got, kernel_mean(P, offset_copy(xd), lsd, ad, offset_copy(xtd))), "scalar load path != 16-byte path"
    assert torch.equal(got, kernel_mean(P, offset_copy(xd), lsd, ad, xtd)) and torch.equal(got, kernel_mean(P, xd, lsd, ad, offset_copy(xtd)))


@pytest.mark.parametrize("d", [5, 8])
def test_mean_batch_split_gives_the_same_bits(P, d):
    x, ls, al, xt = mean_problem(515, 70, d, 9500 + d)
    xd, lsd, ad, xtd = cu(x).contiguous(), lib_ls(ls, LN2), cu(al).contiguous(), cu(xt).contiguous()
    whole = kernel_mean(P, xd, lsd, ad, xtd)
    assert torch.equal(kernel_mean(P, xd, lsd, ad, xtd[3:41]), whole[3:41])  # (aligned or 8 bytes off, as d * 3 falls)
    assert torch.equal(kernel_mean(P, xd, lsd, ad, xtd[69:70]), whole[69:70])


def test_mean_duplicated_and_far_points(P):
    """test points that ARE training points count alpha_j with kappa = 1 exactly; a training point 1e4 lengthscales away
    contributes exactly 0 at alpha = 1e3 and its 3e-6 share at alpha = ln 2"""
    n, t, d = 130, 70, 5
    x, ls, al, xt = mean_problem(n, t, d, 9700)
    xt[0], xt[1], xt[64], xt[69] = x[3], x[64], x[3], x[129]
    x[5] = x[5] + 1e4 * ls
    without = al.clone()
    without[5] = 0.0
    for alpha, dead in ((1e3, True), (LN2, False)):
        want, scale = mean_truth(x, ls, alpha, S_MEAN, MEAN, al, xt)
        got = kernel_mean(P, cu(x), lib_ls(ls, alpha), cu(al), cu(xt))
        check_mean(f"duplicates and a far point alpha={alpha:g}", got, want, scale)
        assert torch.equal(got, kernel_mean(P, cu(x), lib_ls(ls, alpha), cu(without), cu(xt))) == dead, "the far point's share"
        one = kernel_mean(P, cu(x[3:4]), lib_ls(ls, alpha), cu(al[3:4]), cu(xt[:1]), s=1.0, mean=0.0)
        assert one[0].item() == al[3].item(), "one training point met exactly, mean 0, outputscale 1: the result IS alpha_j"
    far = kernel_mean(P, cu(x[5:6]), lib_ls(ls, 1e3), cu(al[5:6]), cu(xt[:3]))
    assert torch.equal(far, torch.full((3,), MEAN, dtype=F64))


def test_predict_mean_is_predict(P):
    x, y, _, _ = T.case_inputs("rq-n65-d3-aln2")
    model = P.pkg.ExactGP(x, y, "rq")
    model.set_raw_parameters(torch.tensor([0.1, -1.5, 0.3, 0.2, 0.6, -0.1, 0.8], dtype=F64))
    xt = torch.randn(40, 3, generator=torch.Generator().manual_seed(23), dtype=F64)
    k = rq_torch(model.lengthscale, model.outputscale, model.alpha)
    ky = k(x, x) + model.noise * torch.eye(65, dtype=F64)
    assert torch.linalg.cond(ky).item() <= 1e3
    low = torch.linalg.cholesky(ky)
    want = model.mean_constant + k(x, xt).T @ torch.cholesky_solve((y - model.mean_constant)[:, None], low)[:, 0]
    want_var = model.outputscale - torch.linalg.solve_triangular(low, k(x, xt), upper=False).square().sum(dim=0)
    mean, var, _ = (v.cpu() for v in model.predict(xt))
    s = model.outputscale
    assert ((mean - want).abs().max() / s).item() <= 1e-11 and ((var - want_var).abs().max() / s).item() <= 1e-10
    assert ((model.predict_mean(xt).cpu() - want).abs().max() / s).item() <= 1e-11


# ---- 5. the selector -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,d", [(200, 12, 2), (1000, 40, 3), (2000, 64, 3)])
def test_conditional_variance_selector(P, n, m, d):
    """The HIP selector with an RQKernel picks exactly the indices of the numpy restatement fed the RQ closure"""
    from oracle import selectors_oracle as SO
    from projected_langevin_sampling_amd.inducing_point_selectors import ConditionalVarianceInducingPointSelector

    g = torch.Generator().manual_seed(n + m)
    x = torch.rand(n, d, generator=g, dtype=F64) * 2 - 1
    ls = 0.4 + torch.rand(d, generator=g, dtype=F64)
    kern = rq_numpy(ls.numpy(), 1.7, 1.5)
    np.random.seed(7)
    x_sel, idx = ConditionalVarianceInducingPointSelector()(x, m, P.pkg.RQKernel(ls, 1.7, alpha=1.5))
    np.random.seed(7)
    _, idx_want, _, _ = SO.conditional_variance_select(x.numpy(), m, kern)
    assert idx.shape == (m,) and len(set(idx.tolist())) == m
    assert np.array_equal(x_sel.numpy(), x.numpy()[idx.numpy()]), "the rows are not the rows of the indices"
    got = idx.numpy()
    assert np.array_equal(got, idx_want), f"picks differ from pick {int(np.argmax(got != idx_want))} on"


# ---- 6. training -----------------------------------------------------------------------------------------------------------
def _training_data(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    y = torch.sin(1.5 * x[:, 0]) + 0.5 * x[:, -1] + 0.2 * torch.randn(n, generator=g, dtype=F64)
    return x, y


def test_training_follows_the_cpu_loop(P):
    """train_exact_gp(kernel="rq") on the library against the same loop with the LAPACK helper as ``evaluate``.  The bar comes
    from the CPU loop alone: rerun with every gradient component perturbed by a relative 1e-12 (alternating signs), 16 x
    the divergence of the losses and of the final raw parameters, floor 1e-11."""
    pkg = P.pkg
    x, y = _training_data(130, 2, 21)
    args = dict(seed=3, number_of_epochs=30, learning_rate=0.05, early_stopper_patience=10.0)

    def perturbed(model):
        loss, grad = T.host_evaluate(model)
        sign = torch.tensor([1.0 if k % 2 == 0 else -1.0 for k in range(grad.numel())], dtype=F64)
        return loss, grad * (1.0 + 1e-12 * sign)

    cpu_model, cpu_losses = pkg.train_exact_gp(x, y, "rq", evaluate=T.host_evaluate, **args)
    per_model, per_losses = pkg.train_exact_gp(x, y, "rq", evaluate=perturbed, **args)
    gpu_model, gpu_losses = pkg.train_exact_gp(x, y, "rq", **args)
    assert len(cpu_losses) == len(per_losses) == len(gpu_losses) == 30
    bar_loss = max(16.0 * np.abs(np.array(cpu_losses) - np.array(per_losses)).max(), 1e-11)
    bar_raw = max(16.0 * (cpu_model.raw_parameters() - per_model.raw_parameters()).abs().max().item(), 1e-11)
    d_loss = np.abs(np.array(cpu_losses) - np.array(gpu_losses)).max()
    d_raw = (cpu_model.raw_parameters() - gpu_model.raw_parameters()).abs().max().item()
    print(f"rq: loss {cpu_losses[0]:.6f} -> {cpu_losses[-1]:.6f}, alpha {LN2:.4f} -> {gpu_model.alpha:.4f}; |gpu - cpu| losses "
          f"{d_loss:.2e} (bar {bar_loss:.2e}), raw {d_raw:.2e} (bar {bar_raw:.2e})")
    note("training", "losses", d_loss / bar_loss)
    note("training", "raw", d_raw / bar_raw)
    assert cpu_losses[-1] < cpu_losses[0] and gpu_losses[-1] < gpu_losses[0]
    assert abs(gpu_model.alpha - LN2) > 1e-3, "test construction: alpha must move"
    assert d_loss <= bar_loss and d_raw <= bar_raw


# ---- 7. steps --------------------------------------------------------------------------------------------------------------
STEP = dict(n=1000, m=40, j=64, d=5, seed=12)  # the smallest problem of the Matern step tests
STEP_S, STEP_ALPHA = 1.3, 1.5


def test_onb_step_against_the_oracle_every_native_cost(P):
    pr = make_problem(STEP["n"], STEP["m"], STEP["j"], STEP["d"], seed=STEP["seed"])
    ob = O.OrthonormalBasis(rq_torch(pr["ls"], STEP_S, STEP_ALPHA), pr["z"], pr["x"], 1e-6)
    lam_all, vec_all = torch.linalg.eigh((1 / pr["z"].shape[0]) * ob.base_gram_induce)
    gb = P.basis.OrthonormalBasis(P.pkg.PLSKernel(P.pkg.RQKernel(pr["ls"], STEP_S, alpha=STEP_ALPHA), pr["z"]), pr["z"], pr["x"], 1e-6,
                                  spectrum=(lam_all, vec_all), verbose=False)
    mk = ob.approximation_dimension
    assert gb.approximation_dimension == mk
    # prior-scaled particles, injected noise, the Poisson particles shifted off the pole of -2 y log|f| (test_gpu_matern)
    u_prior = (pr["u"][:mk] * torch.sqrt(ob.eigenvalues)[:, None]).contiguous()
    xi = torch.randn(mk, STEP["j"], generator=pr["gen"])
    a_or = ob.scaled_eigenvectors.T @ ob.base_gram_induce_train
    e1 = a_or @ torch.ones(STEP["n"])
    u_pos = (e1 * (3.0 / (a_or.T @ e1).mean()))[:, None] + 0.02 * u_prior
    eta, checked = 1e-4, 0
    for name, oc, gc in make_costs(P, pr["y"], pr["fstar"], pr["gen"])[:6]:
        u = u_pos if name.startswith("poisson") else u_prior
        want = O.PLS(ob, oc).calculate_particle_update(u.clone(), eta, noise=xi)
        tol = step_tolerance(ob, oc, u, eta, xi, want)
        assert tol < 1e-8, f"{name}: the problem cannot be held to 1e-8 (tol {tol:.1e})"
        got = gb.fused_step(gc, cu(u), eta, noise=P.basis.NoiseSpec(injected=cu(xi)), force_generic=True)
        err = relerr(got, want)
        note("onb step", f"mk={mk} {name} (tol {tol:.1e})", err / tol)
        assert err < tol, f"{name}: {err:.2e} (tol {tol:.1e})"
        e_want = O.PLS(ob, oc).calculate_energy_potential(u.clone())
        e_got = gb.fused_particle_energy(gc, cu(u), force_generic=True).mean().item()
        assert abs(e_got - e_want) <= max(1e-9, tol) * abs(e_want), name
        if name == "gaussian/identity":
            fast = gb.fused_step(gc, cu(u), eta, noise=P.basis.NoiseSpec(injected=cu(xi)))
            assert relerr(fast, want) < 1e-8, f"fast path: {relerr(fast, want):.2e}"
        checked += 1
    assert checked == 6


def test_ipb_step_against_the_oracle_every_native_cost(P):
    """The six native (cost, link) pairs with condition-scaled tolerances; the Poisson pair may be skipped where the
    oracle alone shows that no fp64 implementation holds it to 1e-8 (the existing rule), and the count is asserted."""
    pr = make_problem(STEP["n"], STEP["m"], STEP["j"], STEP["d"], seed=STEP["seed"])
    m = STEP["m"]
    yz = pr["y"][:m]
    ob = O.InducingPointBasis(rq_torch(pr["ls"], STEP_S, STEP_ALPHA), pr["z"], yz, pr["x"])
    cond = torch.linalg.cond(ob.base_gram_induce).item()
    gb = P.basis.InducingPointBasis(P.pkg.PLSKernel(P.pkg.RQKernel(pr["ls"], STEP_S, alpha=STEP_ALPHA), pr["z"]), pr["z"], yz, pr["x"])
    u = pr["u"]
    e_noise = torch.randn(m, STEP["j"], generator=pr["gen"])
    eta, checked, skipped = 1e-4, 0, []
    for name, oc, gc in make_costs(P, pr["y"], pr["fstar"], pr["gen"])[:6]:
        want = O.PLS(ob, oc).calculate_particle_update(u.clone(), eta, noise=e_noise)
        tol = step_tolerance(ob, oc, u, eta, e_noise, want, solve_cond=cond)
        if name.startswith("poisson") and tol >= 1e-8:
            skipped.append((name, f"{tol:.1e}"))
            continue
        got = gb.fused_step(gc, cu(u), eta, noise=P.basis.NoiseSpec(injected=cu(e_noise)), force_generic=True)
        err = relerr(got, want)
        note("ipb step", f"m={m} {name} (tol {tol:.1e}, cond {cond:.1e})", err / tol)
        assert err < tol, f"{name} (cond {cond:.1e}): {err:.2e} (tol {tol:.1e})"
        e_want = O.PLS(ob, oc).calculate_energy_potential(u.clone())
        assert abs(P.pkg.PLS(gb, gc).calculate_energy_potential(cu(u)) - e_want) <= max(1e-9, tol) * abs(e_want), name
        if name == "gaussian/identity":
            fast = gb.fused_step(gc, cu(u), eta, noise=P.basis.NoiseSpec(injected=cu(e_noise)))
            assert relerr(fast, want) < 1e-8, f"M x M x J path: {relerr(fast, want):.2e}"
        checked += 1
    print(f"ipb step: {checked} of 6 pairs held to the oracle; skipped for conditioning: {skipped}")
    assert checked >= 5 and len(skipped) <= 1


# ---- 8. the hand-over ------------------------------------------------------------------------------------------------------
def test_hand_over_to_pls_training(P):
    """exact_gp_runner(kernel="rq") -> construct_average_ard_kernel -> selector -> PLSKernel -> one train_pls iteration"""
    pkg = P.pkg
    from projected_langevin_sampling_amd.basis import OrthonormalBasis
    from projected_langevin_sampling_amd.costs import GaussianCost
    from projected_langevin_sampling_amd.inducing_point_selectors import ConditionalVarianceInducingPointSelector
    from projected_langevin_sampling_amd.link_functions import IdentityLinkFunction

    x, y = _training_data(600, 3, 24)
    models = pkg.exact_gp_runner(x, y, "rq", subsample_size=200, seed=5, number_of_epochs=5, learning_rate=0.05,
                                 number_of_iterations=2, early_stopper_patience=10.0)
    assert len(models) == 2 and all(m.n == 200 and m.kind == RQ for m in models)
    kernel = pkg.construct_average_ard_kernel(models)
    noise = pkg.construct_average_gaussian_noise(models)
    sp = torch.nn.functional.softplus
    assert type(kernel) is pkg.RQKernel and kernel.lengthscale.numel() == 3 and noise > 1e-4
    assert kernel.alpha == float(sp(torch.stack([m.raw_parameters()[-1] for m in models]).mean())) != LN2
    np.random.seed(3)
    z, _ = ConditionalVarianceInducingPointSelector()(x, 24, kernel)
    assert z.shape == (24, 3)
    basis = OrthonormalBasis(pkg.PLSKernel(kernel, z), z, x, 1e-6, verbose=False)
    pls = pkg.PLS(basis, GaussianCost(noise, y, IdentityLinkFunction()))
    u = torch.randn(basis.approximation_dimension, 16, generator=torch.Generator().manual_seed(25), dtype=F64).cuda()
    update = pls.calculate_particle_update(u, 1e-3)
    assert update.shape == u.shape and torch.isfinite(update).all()
    particles = pls.initialise_particles(number_of_particles=16, seed=4)
    final, energies = pkg.train_pls(pls, particles, number_of_epochs=1, step_size=1e-3, early_stopper_patience=10.0)
    assert final.shape == (basis.approximation_dimension, 16) and torch.isfinite(final).all() and len(energies) == 1


def test_svgp_on_a_pls_kernel_of_an_rq_kernel(P):
    """SVGP(PLSKernel(RQKernel), ...).fit_data and one elbo_and_grad against the svgp_truth helper given the closed-form Gram
    matrices.  The bar, relative to each output's sum of magnitudes: svgp_truth.bar's roundings per output, plus what the
    Cholesky solve leaves in the rows a_i of L^-1 r(Z, x), c = cond(K_zz + jitter I) eps relative: q_i = r_ii + jitter -
    |a_i|^2 moves by 2 c |a_i|^2 <= 2 c s, which the log-likelihood divides by 2 noise = 0.14 -- 17 c against a sum of
    magnitudes of order 1; 32 c allowed."""
    pkg = P.pkg
    n, m = 130, 12
    g = torch.Generator().manual_seed(43)
    x = torch.rand(n, 2, generator=g, dtype=F64) * 2 - 1
    y = torch.sin(3.0 * x[:, 0]) + 0.1 * torch.randn(n, generator=g, dtype=F64)
    z = x[:m].clone()
    ls, s, alpha, jitter = torch.tensor([0.3, 0.4], dtype=F64), 1.2, 0.8, 1e-6
    model = pkg.SVGP(pkg.PLSKernel(pkg.RQKernel(ls, s, alpha=alpha), z), z, noise=0.07, mean_constant=0.1).fit_data(x, y)
    inp = ST.make_inputs(44, n, m)
    model.variational_mean.copy_(inp["mean"])
    model.chol_variational_covar.copy_(torch.tril(inp["Ls"]))
    k = rq_torch(ls, s, alpha)
    s_unique = z.unique(dim=0)

    def r(a, b):
        return k(a, s_unique) @ k(b, s_unique).T / s_unique.shape[0]

    kzz = r(z, z) + jitter * torch.eye(m, dtype=F64)
    cond = torch.linalg.cond(kzz).item()
    assert cond <= 1e6, f"test construction: cond {cond:.1e}"
    low = torch.linalg.cholesky(kzz)
    a = torch.linalg.solve_triangular(low, r(z, x), upper=False)  # (M, n)
    q = r(x, x).diagonal() + jitter - a.square().sum(dim=0)
    rho = math.log(math.expm1(0.07 - ST.MIN_NOISE))  # noise = softplus(rho) + 1e-4
    args = (a.T.contiguous(), q, y, inp["mean"], inp["Ls"], 0.1, rho, None, n)
    want, scale = ST.evaluate(*args), ST.evaluate(*args, majorant=True)
    elbo, grads = model.elbo_and_grad()
    gl = grads["chol_variational_covar"].cpu().numpy()
    got = np.concatenate([[elbo, grads["mean_constant"], grads["raw_noise"]], grads["variational_mean"].cpu().numpy(), ST.lower_entries(gl)])
    keep = np.r_[0:3, 5:want.size]
    err = np.abs(got - want[keep]) / scale[keep]
    bar = ST.bar(m, n) + 32.0 * cond * ST.EPS
    note("svgp", f"m={m} n={n} cond {cond:.1e}", err.max() / bar)
    assert np.isfinite(got).all() and np.all(err <= bar), err / bar
