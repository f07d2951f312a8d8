"""GPU: pls_kernel_mean, the exact-GP predictive mean without the cross-Gram matrix, through the C ABI -- per test point
against math.fsum of the closed-form terms (every D_MAX instantiation, a second chunk of training points, a second tile
of test points, all four kinds), both load paths, batch-split invariance, duplicated and far-apart points."""
import numpy as np
import pytest
import torch

import student_noise_truth as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
S, MEAN = 1.7, 0.3
# n = 1: a lone training point; 2; 65: a second block of 64 with one row; 515: a second chunk of 512 with an odd tail.
# t = 1: a lone test point; 2; 65: a second tile of one point; 130: a third tile of two
SIZES = [(n, t) for n in (1, 2, 65, 515) for t in (1, 2, 65, 130)]
DIMS = [1, 2, 3, 5, 8, 13, 33, 64]  # every D_MAX: 1, 2, 4, 8, 16, 32, 64, padded and exact
KIND_IDS = [T.KIND_NAMES[k] for k in T.KINDS]
ratios = {}


@pytest.fixture(scope="module")
def lib():
    import projected_langevin_sampling_amd as pkg

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return pkg._lib.load()


def cu(t):
    return t.to(device="cuda", dtype=F64).contiguous()


def offset_copy(m):
    """a device copy of the matrix 8 bytes past a 16-byte boundary"""
    raw = torch.full((1 + m.numel(),), float("nan"), dtype=F64, device="cuda")
    view = raw[1:].view(m.shape)
    view.copy_(m)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


def kernel_mean(lib, kind, xd, lsd, ad, xtd, s=S, mean=MEAN):
    """pls_kernel_mean through the C ABI on device tensors; the output is one element longer, NaN, and the pad is checked"""
    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    (n, d), t = xd.shape, xtd.shape[0]
    out = torch.full((t + 1,), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_mean(kind, xd.data_ptr(), n, d, lsd.data_ptr(), float(s), float(mean), ad.data_ptr(), xtd.data_ptr(), t,
                                out.data_ptr(), L.stream_ptr()), "pls_kernel_mean")
    host = out.cpu()
    assert torch.isnan(host[t]), "pls_kernel_mean wrote past its t outputs"
    return host[:t]


def problem(kind, n, t, d, seed):
    """the distribution of test_gpu_exact_gp.reduction_problem: x ~ N(0, 1), lengthscales (0.5 - 1.5) sqrt(d)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g, dtype=F64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
    alpha = torch.randn(n, generator=g, dtype=F64)
    xt = torch.randn(t, d, generator=g, dtype=F64)
    return x, ls, alpha, xt


def check(tag, got, want, scale):
    ratio = np.abs(got.numpy() - want) / np.where(scale > 0, scale, 1.0)
    ratios[tag] = ratio.max()
    print(f"{tag}: |got - want| / S_i per test point, max {ratio.max():.2e} (largest so far {max(ratios.values()):.2e})")
    assert np.all(np.isfinite(got.numpy())), (tag, got)
    assert np.all(np.abs(got.numpy() - want) <= 1e-13 * scale), (tag, ratio.max())


@pytest.mark.parametrize("kind", T.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n,t,d", [(n, t, 5) for n, t in SIZES] + [(130, 70, d) for d in DIMS])
def test_mean_per_point(lib, kind, n, t, d):
    x, ls, alpha, xt = problem(kind, n, t, d, 9000 + 100 * n + 10 * t + d + kind)
    want, scale = T.kernel_mean(kind, x, ls, S, MEAN, alpha, xt)
    xd, lsd, ad, xtd = cu(x), cu(ls), cu(alpha), cu(xt)
    assert xd.data_ptr() % 16 == 0 and xtd.data_ptr() % 16 == 0
    got = kernel_mean(lib, kind, xd, lsd, ad, xtd)
    check(f"{T.KIND_NAMES[kind]} n={n} t={t} d={d}", got, want, scale)
    assert torch.equal(got, kernel_mean(lib, kind, xd, lsd, ad, xtd)), "two calls differ"
    # both x and xt 8 bytes past a 16-byte boundary: the scalar load paths give the same bits
    assert torch.equal(got, kernel_mean(lib, kind, offset_copy(xd), lsd, ad, offset_copy(xtd))), "scalar load path != 16-byte path"
    assert torch.equal(got, kernel_mean(lib, kind, offset_copy(xd), lsd, ad, xtd)) and torch.equal(
        got, kernel_mean(lib, kind, xd, lsd, ad, offset_copy(xtd)))


@pytest.mark.parametrize("kind", T.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("d", [5, 8])
def test_batch_split_gives_the_same_bits(lib, kind, d):
    """rows 3..40 of a 70-point batch on their own equal the same rows of the whole call, bit for bit"""
    x, ls, alpha, xt = problem(kind, 515, 70, d, 9500 + d + kind)
    xd, lsd, ad, xtd = cu(x), cu(ls), cu(alpha), cu(xt)
    whole = kernel_mean(lib, kind, xd, lsd, ad, xtd)
    part = kernel_mean(lib, kind, xd, lsd, ad, xtd[3:41])
    assert torch.equal(part, whole[3:41])
    assert torch.equal(kernel_mean(lib, kind, xd, lsd, ad, xtd[69:70]), whole[69:70])


@pytest.mark.parametrize("kind", T.KINDS, ids=KIND_IDS)
def test_duplicated_and_far_points(lib, kind):
    """test points that ARE training points count alpha_j with kappa = 1 (nu = 1/2 included: no 1/t), a training point
    1e4 lengthscales away contributes exactly 0; nothing becomes NaN"""
    n, t, d = 130, 70, 5
    x, ls, alpha, xt = problem(kind, n, t, d, 9700 + kind)
    xt[0], xt[1], xt[64], xt[69] = x[3], x[64], x[3], x[129]
    x[5] = x[5] + 1e4 * ls
    want, scale = T.kernel_mean(kind, x, ls, S, MEAN, alpha, xt)
    without = alpha.clone()
    without[5] = 0.0
    assert np.array_equal(want, T.kernel_mean(kind, x, ls, S, MEAN, without, xt)[0]), "the far point's term is not 0 in the truth"
    got = kernel_mean(lib, kind, cu(x), cu(ls), cu(alpha), cu(xt))
    check(f"{T.KIND_NAMES[kind]} duplicates and a far point", got, want, scale)
    assert torch.equal(got, kernel_mean(lib, kind, cu(x), cu(ls), cu(without), cu(xt))), "the far point contributes"
    # one training point met exactly, mean 0, outputscale 1: the result IS alpha
    one = kernel_mean(lib, kind, cu(x[3:4]), cu(ls), cu(alpha[3:4]), cu(xt[:1]), s=1.0, mean=0.0)
    assert one[0].item() == alpha[3].item()
    # ... and with every training point far away the result is the mean itself
    far = kernel_mean(lib, kind, cu(x[5:6]), cu(ls), cu(alpha[5:6]), cu(xt[:3]))
    assert torch.equal(far, torch.full((3,), MEAN, dtype=F64))
