"""CPU: one statement of a base-kernel family's layout -- _lib.kernel_shape_params against the library's own count (the
workspace query of the gradient reduction, which runs before any HIP call), and against every width the Python layer derives
from it: what a kernel object hands the library, what the exact-GP classes hand it, the raw parameters and chain_rule."""
import pytest
import torch

import projected_langevin_sampling_amd as pkg

L = pkg._lib
F64 = torch.float64
#: kind -> (the kernel class, its extra constructor keywords, the name or class the model classes take)
FAMILIES = {
    L.KERNEL_RBF_ARD: (pkg.ARDKernel, {}, "rbf"),
    L.KERNEL_MATERN12: (pkg.MaternKernel, {"nu": 0.5}, "matern12"),
    L.KERNEL_MATERN32: (pkg.MaternKernel, {"nu": 1.5}, "matern32"),
    L.KERNEL_MATERN52: (pkg.MaternKernel, {"nu": 2.5}, "matern52"),
    L.KERNEL_RQ: (pkg.RQKernel, {"alpha": 0.7}, "rq"),
    L.KERNEL_PERIODIC: (pkg.PeriodicKernel, {"period_length": [1.5, 0.5, 2.0]}, pkg.PeriodicKernel),
}
KINDS = list(FAMILIES)


@pytest.mark.parametrize("kind", KINDS)
def test_the_count_is_the_librarys(kind):
    """one partial row of d + 1 + shape parameters doubles per workgroup of 512 x 64 pairs (csrc/base_kernel.h)"""
    assert L.kernel_shape_params(kind, 1) == {L.KERNEL_RQ: 1, L.KERNEL_PERIODIC: 1}.get(kind, 0)
    for n, d in ((515, 5), (130, 16)):
        blocks = -(-n // 512) * -(-n // 64)
        got = L.load().pls_kernel_grad_sums_workspace_bytes_kind(kind, n, d)
        assert got == 8 * blocks * (d + 1 + L.kernel_shape_params(kind, d)), (n, d)


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_width_follows_the_count(kind, ard):
    d, nls = 3, 3 if ard else 1
    cls, keywords, name = FAMILIES[kind]
    count = L.kernel_shape_params(kind, d)
    if not ard and "period_length" in keywords:
        keywords = {"period_length": 1.5}
    start = cls([0.5, 2.0, 1.25] if ard else [0.75], 1.7, **keywords)
    assert start.kind == kind and start._lengthscale_host(d).shape == (d + count,)
    g = torch.Generator().manual_seed(kind)
    x, y = torch.randn(12, d, generator=g, dtype=F64), torch.randn(12, generator=g, dtype=F64)
    for kernel in (name, start):
        model = pkg.ExactGP(x, y, kernel=kernel, ard=ard)
        assert model.kind == kind and model.ard == ard
        assert model._library_lengthscale().shape == (1, d + count)
        # the documented width: mean, raw noise, raw outputscale, nls raw lengthscales, then the raw shape values -- one
        # per library value, a per-dimension one shared when the lengthscale is
        assert model.raw.numel() == 3 + nls + L.kernel_shape_params(kind, nls)
        out = torch.randn(4 + d + count, generator=g, dtype=F64)
        loss, grad = model.chain_rule(out)
        assert grad.shape == model.raw.shape and torch.isfinite(grad).all() and loss == -out[0].item() / 12
        with pytest.raises(AssertionError):
            model.chain_rule(out[:-1])
        if kernel is start:
            assert torch.allclose(model._library_lengthscale()[0], start._lengthscale_host(d), rtol=1e-14, atol=0)
