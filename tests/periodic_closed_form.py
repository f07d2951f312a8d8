"""Closed form of gpytorch's ScaleKernel(PeriodicKernel) with ARD lengthscales and period lengths (as recalled -- a reading,
not a run of gpytorch; include/plship.h states the formula and it is the contract), the yardstick of the periodic tests.

With e_k = (a_k - b_k) / p_k from direct differences, the lengthscales lambda_k (they divide and are not squared), the period
lengths p_k and the outputscale s,
    k = s * exp(-2 sum_k sin^2(pi e_k) / lambda_k).
The sine is taken of the REDUCED argument, r = e - rint(e) with |r| <= 1/2 (exact in float64), so that a large e keeps the
digits it has: sin(pi r) = +-sin(pi e).  k(x, x) = s exactly; a non-finite difference gives NaN (no limit at infinity).

``periodic_torch`` is a base-kernel callable for the CPU oracle (oracle.pls_oracle), ``periodic_numpy`` one for
oracle.selectors_oracle; ``periodic_factors_numpy`` gives kappa and the derivative factors of pairs from their differences,
``sensitivity`` the first-order sensitivity c of the exponent to a relative error in the e_k."""
import numpy as np
import torch

LN2 = 0.6931471805599453  # lengthscale and period length at raw value 0


def periodic_factors_numpy(delta, lengthscale, period):
    """(kappa (...), fl (..., d), fp (..., d), e (..., d)) of pairs with differences delta (..., d):
    fl_k = (2 / lambda_k) sin^2(pi e_k)              d kappa / d log lambda_k = kappa fl_k
    fp_k = (2 / lambda_k) pi e_k sin(2 pi e_k)       d kappa / d log p_k      = kappa fp_k
    and kappa = exp(-sum_k fl_k)."""
    delta = np.asarray(delta, dtype=np.float64)
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    period = np.asarray(period, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", under="ignore"):
        e = delta / period
        r = e - np.rint(e)
        s, c = np.sin(np.pi * r), np.cos(np.pi * r)
        fl = (2.0 / ls) * (s * s)
        fp = (2.0 / ls) * (np.pi * e) * (2.0 * s * c)
        return np.exp(-fl.sum(-1)), fl, fp, e


def sensitivity(e, lengthscale):
    """c = 1 + sum_k (2 pi / lambda_k) |e_k|: a relative error eps in every e_k moves the exponent by at most (c - 1) eps"""
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    return 1.0 + ((2.0 * np.pi / ls) * np.abs(np.asarray(e, dtype=np.float64))).sum(-1)


def periodic_numpy(lengthscale, outputscale=1.0, period=1.0):
    def k(x1, x2):
        delta = np.asarray(x1, dtype=np.float64)[:, None, :] - np.asarray(x2, dtype=np.float64)[None, :, :]
        return float(outputscale) * periodic_factors_numpy(delta, lengthscale, period)[0]

    return k


def periodic_torch(lengthscale, outputscale=1.0, period=1.0):
    ls = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1)
    period = torch.as_tensor(period, dtype=torch.float64).reshape(-1)

    def k(x1, x2):
        x1 = x1 if x1.dim() == 2 else x1[:, None]
        x2 = x2 if x2.dim() == 2 else x2[:, None]
        e = (x1[:, None, :].double() - x2[None, :, :].double()) / period
        r = e - torch.round(e)
        return float(outputscale) * torch.exp(-(2.0 / ls * torch.sin(torch.pi * r).square()).sum(-1))

    return k
