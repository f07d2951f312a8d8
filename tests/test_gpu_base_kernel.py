"""GPU: the three pairwise entries see the same kappa, bit for bit.  The exact-GP path builds K with pls_kernel_gram,
differentiates with pls_kernel_grad_sums and predicts with pls_kernel_mean; all three take kappa from pair_kappa
(csrc/kernel_math.h) over the same pre-scaled distance sum (csrc/base_kernel.h).  With K = pls_kernel_gram(x, xt) at
outputscale 1:
  * pls_kernel_mean with the single training point x[j], alpha = 1, mean = 0, outputscale 1 returns K[j, i]: the one term
    fma(kappa, 1, 0), the other waves' sums exact zeros, fma(1, sum, 0);
  * pls_kernel_grad_sums on the two points (x[j], xt[i]) with alpha = 0 and P zero but for P[0][1] = -1 returns
    out[0] = K[j, i]: W = 0 * 0 - P is 1 at (0, 1) and 0 elsewhere, so the sum is fma(1, kappa, 0) plus exact zeros.
The pairs include a duplicate (kappa exactly 1 in all three) and a point 1e4 lengthscales away (exactly 0 in all three)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F64 = torch.float64
KINDS = {0: "rbf", 2: "matern12", 3: "matern32", 4: "matern52"}
DIMS = (1, 3, 8, 33)  # D_MAX 1, 4 (padded), 8 (exact), 64 (padded)
DUPLICATE, FAR = (1, 0), 1  # xt[0] is x[1]; xt[1] is far from every x[j]


@pytest.fixture(scope="module")
def lib():
    import projected_langevin_sampling_amd as pkg

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return pkg._lib.load()


def points(kind, d):
    """x (3, d) ~ N(0, 1), lengthscales (0.5 - 1.5) sqrt(d); xt (3, d): x[1] again, x[0] moved by 1e4 lengthscales in
    every coordinate, a fresh point"""
    g = torch.Generator().manual_seed(4100 + 10 * d + kind)
    x = torch.randn(3, d, generator=g, dtype=F64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=F64)) * d**0.5
    xt = torch.stack([x[1], x[0] + 1e4 * ls, torch.randn(d, generator=g, dtype=F64)])
    return x.cuda(), ls.cuda(), xt.cuda()


def gram(lib, L, kind, x, ls, xt):
    out = torch.full((x.shape[0], xt.shape[0]), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_gram(kind, x.data_ptr(), x.shape[0], xt.data_ptr(), xt.shape[0], x.shape[1], ls.data_ptr(), 1.0,
                                out.data_ptr(), xt.shape[0], L.stream_ptr()), "pls_kernel_gram")
    return out.cpu()


def mean_of_one(lib, L, kind, xj, ls, xt):
    """pls_kernel_mean with the one training point xj (1, d), alpha = 1, mean = 0, outputscale 1, at every xt"""
    one = torch.ones(1, dtype=F64, device="cuda")
    out = torch.full((xt.shape[0],), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_mean(kind, xj.data_ptr(), 1, xj.shape[1], ls.data_ptr(), 1.0, 0.0, one.data_ptr(), xt.data_ptr(),
                                xt.shape[0], out.data_ptr(), L.stream_ptr()), "pls_kernel_mean")
    return out.cpu()


def grad_sum_of_one(lib, L, kind, xj, xti, ls):
    """out[0] of pls_kernel_grad_sums on the two points (xj, xti) with alpha = 0 and P = 0 but for P[0][1] = -1"""
    d = xj.shape[0]
    pair = torch.stack([xj, xti]).contiguous()
    alpha = torch.zeros(2, dtype=F64, device="cuda")
    p = torch.zeros(2, 2, dtype=F64, device="cuda")
    p[0, 1] = -1.0
    nbytes = lib.pls_kernel_grad_sums_workspace_bytes(2, d)
    ws = torch.empty(nbytes // 8, dtype=F64, device="cuda")
    out = torch.full((d + 1,), float("nan"), dtype=F64, device="cuda")
    L.check(lib.pls_kernel_grad_sums(kind, pair.data_ptr(), 2, d, ls.data_ptr(), 1.0, alpha.data_ptr(), p.data_ptr(), 2,
                                     out.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr()), "pls_kernel_grad_sums")
    return out.cpu()[0]


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", list(KINDS), ids=list(KINDS.values()))
def test_the_three_entries_see_the_same_kappa(lib, kind, d):
    import projected_langevin_sampling_amd as pkg

    L = pkg._lib
    x, ls, xt = points(kind, d)
    k = gram(lib, L, kind, x, ls, xt)
    mean = torch.stack([mean_of_one(lib, L, kind, x[j : j + 1], ls, xt) for j in range(x.shape[0])])
    sums = torch.stack([torch.stack([grad_sum_of_one(lib, L, kind, x[j], xt[i], ls) for i in range(xt.shape[0])])
                        for j in range(x.shape[0])])
    print(f"{KINDS[kind]} d={d}: K =\n{k}\nmean - K =\n{mean - k}\ngrad_sums - K =\n{sums - k}")
    assert torch.isfinite(k).all() and (k[:, 2] > 0).all() and (k[:, 2] < 1).all(), k  # (the fresh point: an ordinary pair)
    assert torch.equal(mean, k), (mean - k)
    assert torch.equal(sums, k), (sums - k)
    for name, got in (("gram", k), ("mean", mean), ("grad_sums", sums)):
        assert torch.equal(got[:, FAR], torch.zeros(x.shape[0], dtype=F64)), (name, got[:, FAR])
        assert got[DUPLICATE].item() == 1.0, (name, got[DUPLICATE].item())
