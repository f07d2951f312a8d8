"""CPU: the host side of the Matern base kernels -- gpytorch-shaped objects read by as_base_kernel, the C ABI's argument
checks for the Matern kinds (they run before any HIP call), and the closed-form yardstick against 40-digit arithmetic."""
import numpy as np
import pytest
import torch

import projected_langevin_sampling_amd as pkg
from matern_closed_form import NUS, matern_numpy, matern_torch
from projected_langevin_sampling_amd.kernel import ARDKernel, MaternKernel, as_base_kernel

L = pkg._lib


def _scale_stub(lengthscale, outputscale, nu=None):
    """A gpytorch ScaleKernel(MaternKernel(nu)) as the reference would hand it over (nu=None: ScaleKernel(RBFKernel))."""
    inner = type("Inner", (), {"lengthscale": lengthscale})()
    if nu is not None:
        inner.nu = nu
    return type("ScaleStub", (), {"base_kernel": inner, "outputscale": outputscale})()


@pytest.mark.parametrize("nu,kind", [(0.5, L.KERNEL_MATERN12), (1.5, L.KERNEL_MATERN32), (2.5, L.KERNEL_MATERN52)])
def test_as_base_kernel_reads_a_scale_matern_kernel(nu, kind):
    k = as_base_kernel(_scale_stub(torch.tensor([[0.5, 2.0, 1.25]]), torch.tensor(3.0), nu))
    assert type(k) is MaternKernel and k.kind == kind and k.nu == nu
    assert k.lengthscale.tolist() == [0.5, 2.0, 1.25] and k.outputscale == 3.0
    k = as_base_kernel(_scale_stub(torch.tensor([[0.75]]), 1.5, nu))  # one shared lengthscale, a float outputscale
    assert type(k) is MaternKernel and k.kind == kind and k.lengthscale.tolist() == [0.75] and k.outputscale == 1.5
    assert MaternKernel([0.5, 2.0], 2.0, nu=nu).kind == kind
    assert as_base_kernel(k) is k


def test_matern_nu_outside_gpytorchs_three_is_refused():
    with pytest.raises(ValueError, match="nu"):
        as_base_kernel(_scale_stub(torch.tensor([[1.0]]), torch.tensor(1.0), 2.0))
    with pytest.raises(ValueError, match="nu"):
        MaternKernel([1.0], 1.0, nu=2.0)
    assert MaternKernel([1.0]).kind == L.KERNEL_MATERN52  # gpytorch's default nu = 2.5


def test_a_stub_without_nu_is_still_read_as_rbf():
    k = as_base_kernel(_scale_stub(torch.tensor([[0.5, 2.0]]), torch.tensor(3.0)))
    assert type(k) is ARDKernel and k.kind == L.KERNEL_RBF_ARD and k.outputscale == 3.0 and k.lengthscale.tolist() == [0.5, 2.0]


def test_cabi_matern_kinds_need_a_lengthscale():
    """Validation before any HIP call: kinds 2-4 exist (the parent library called them unknown) and need a lengthscale;
    kind 5 does not exist."""
    lib = L.load()
    assert lib.pls_abi_version() == 7
    for kind in (L.KERNEL_MATERN12, L.KERNEL_MATERN32, L.KERNEL_MATERN52):
        assert lib.pls_kernel_gram(kind, 8, 1, 8, 1, 1, None, 1.0, 8, 1, None) == 1
        msg = lib.pls_last_error()
        assert b"lengthscale" in msg and b"unknown" not in msg, msg
        assert lib.pls_select_inducing_conditional_variance(kind, 8, 4, 1, None, 1.0, 2, 1e-12, 0.0, 8, 8, None, 0, None) == 1
        msg = lib.pls_last_error()
        assert b"lengthscale" in msg and b"unknown" not in msg, msg
    assert lib.pls_kernel_gram(5, 8, 1, 8, 1, 1, 8, 1.0, 8, 1, None) == 1
    assert b"unknown kernel kind" in lib.pls_last_error()
    assert lib.pls_select_inducing_conditional_variance(5, 8, 4, 1, 8, 1.0, 2, 1e-12, 0.0, 8, 8, None, 0, None) == 1
    assert b"unknown kernel kind" in lib.pls_last_error()


@pytest.mark.parametrize("d", [1, 3, 8, 13, 64])
def test_closed_forms_against_40_digits(d):
    """Both closed forms (torch and numpy) within a relative error of 1e-15 of the same formula evaluated at 40 digits from
    the same fp64 inputs; k(x, x) is the outputscale exactly.  Relative error as everywhere in this suite (relerr in
    test_gpu_parity.py): the largest absolute error over the largest entry.  (Per entry, the error of t = sqrt(2 nu) r,
    a few ulp of t, turns into a relative error of t ulp in exp(-t): up to 1.4e-15 on these inputs.)"""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 40
    g = torch.Generator().manual_seed(100 + d)
    x1, x2 = torch.randn(7, d, generator=g, dtype=torch.float64), torch.randn(9, d, generator=g, dtype=torch.float64)
    ls = (0.5 + torch.rand(d, generator=g, dtype=torch.float64)) * d**0.5  # r = O(1)
    s = 2.5
    a, b, l = x1.numpy(), x2.numpy(), ls.numpy()
    for nu in NUS:
        c = mpmath.sqrt(2 * mpmath.mpf(nu))
        want = np.empty((7, 9))
        for i in range(7):
            for j in range(9):
                r = mpmath.sqrt(mpmath.fsum(((mpmath.mpf(a[i, k]) - mpmath.mpf(b[j, k])) / mpmath.mpf(l[k])) ** 2 for k in range(d)))
                t = c * r
                p = 1 if nu == 0.5 else (1 + t if nu == 1.5 else 1 + t + t * t / 3)
                want[i, j] = float(s * p * mpmath.exp(-t))
        for got in (matern_torch(ls, s, nu)(x1, x2).numpy(), matern_numpy(l, s, nu)(a, b)):
            err = np.abs(got - want).max() / np.abs(want).max()
            print(f"nu={nu} d={d}: rel err vs 40 digits {err:.2e} (per entry {(np.abs(got - want) / np.abs(want)).max():.2e})")
            assert err <= 1e-15, (nu, d, err)
        assert np.all(matern_torch(ls, s, nu)(x1, x1).diagonal().numpy() == s)
        assert np.all(np.diag(matern_numpy(l, s, nu)(a, a)) == s)
