"""Closed form of gpytorch's ScaleKernel(RBFKernel * PeriodicKernel) with ARD parameters, the locally periodic kernel (as
recalled -- a reading, not a run of gpytorch; include/plship.h states the formula and it is the contract), the yardstick of
the locally periodic tests.

With direct differences delta_k = a_k - b_k, the envelope lengthscales l_k, the periodic lengthscales lambda_k (they divide and
are not squared), the period lengths p_k, e_k = delta_k / p_k and the outputscale s,
    k = s * exp(-(1/2 sum_k (delta_k / l_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k)).
The sine is taken of the REDUCED argument, as periodic_closed_form does.  k(x, x) = s exactly; a non-finite difference gives
NaN.

``locally_periodic_torch`` is a base-kernel callable for the CPU oracle (oracle.pls_oracle), ``locally_periodic_numpy`` one
for oracle.selectors_oracle; ``locally_periodic_factors_numpy`` gives kappa and the derivative factors of pairs from their
differences, ``sensitivity`` the first-order sensitivity c of the exponent to a relative error in the differences."""
import numpy as np
import torch

from periodic_closed_form import LN2, periodic_factors_numpy  # noqa: F401


def locally_periodic_factors_numpy(delta, lengthscale, periodic_lengthscale, period):
    """(kappa (...), fe (..., d), fl (..., d), fp (..., d), e (..., d)) of pairs with differences delta (..., d):
    fe_k = (delta_k / l_k)^2                         d kappa / d log l_k      = kappa fe_k
    fl_k = (2 / lambda_k) sin^2(pi e_k)              d kappa / d log lambda_k = kappa fl_k
    fp_k = (2 / lambda_k) pi e_k sin(2 pi e_k)       d kappa / d log p_k      = kappa fp_k
    and kappa = exp(-sum_k (fe_k / 2 + fl_k))."""
    delta = np.asarray(delta, dtype=np.float64)
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    _, fl, fp, e = periodic_factors_numpy(delta, periodic_lengthscale, period)
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        fe = np.square(delta / ls)
        return np.exp(-(0.5 * fe + fl).sum(-1)), fe, fl, fp, e


def sensitivity(delta, e, lengthscale, periodic_lengthscale):
    """c = 1 + r^2 + sum_k (2 pi / lambda_k) |e_k| with r^2 = sum_k (delta_k / l_k)^2: a relative error eps in every
    difference moves the exponent by at most (c - 1) eps -- the envelope's share r^2 / 2 by r^2 eps, the periodic share as
    periodic_closed_form.sensitivity has it"""
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    lam = np.asarray(periodic_lengthscale, dtype=np.float64).reshape(-1)
    r2 = np.square(np.asarray(delta, dtype=np.float64) / ls).sum(-1)
    return 1.0 + r2 + ((2.0 * np.pi / lam) * np.abs(np.asarray(e, dtype=np.float64))).sum(-1)


def locally_periodic_numpy(lengthscale, outputscale=1.0, periodic_lengthscale=1.0, period=1.0):
    def k(x1, x2):
        delta = np.asarray(x1, dtype=np.float64)[:, None, :] - np.asarray(x2, dtype=np.float64)[None, :, :]
        return float(outputscale) * locally_periodic_factors_numpy(delta, lengthscale, periodic_lengthscale, period)[0]

    return k


def locally_periodic_torch(lengthscale, outputscale=1.0, periodic_lengthscale=1.0, period=1.0):
    ls = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1)
    lam = torch.as_tensor(periodic_lengthscale, dtype=torch.float64).reshape(-1)
    period = torch.as_tensor(period, dtype=torch.float64).reshape(-1)

    def k(x1, x2):
        x1 = x1 if x1.dim() == 2 else x1[:, None]
        x2 = x2 if x2.dim() == 2 else x2[:, None]
        delta = x1[:, None, :].double() - x2[None, :, :].double()
        e = delta / period
        r = e - torch.round(e)
        return float(outputscale) * torch.exp(-(0.5 * (delta / ls).square() + 2.0 / lam * torch.sin(torch.pi * r).square()).sum(-1))

    return k
