"""Closed form of gpytorch's ScaleKernel(RBFKernel) + ScaleKernel(RBFKernel * PeriodicKernel) with ARD parameters, the
trend-plus-seasonal kernel (as recalled -- a reading, not a run of gpytorch; include/plship.h states the formula and it is the
contract), the yardstick of the trend-plus-seasonal tests.

With direct differences delta_k = a_k - b_k, the trend lengthscales l_k and outputscale s_t, the seasonal term's envelope
lengthscales m_k, periodic lengthscales lambda_k (they divide and are not squared), period lengths p_k, e_k = delta_k / p_k and
outputscale s_s,
    k = s_t exp(-1/2 sum_k (delta_k / l_k)^2) + s_s exp(-(1/2 sum_k (delta_k / m_k)^2 + 2 sum_k sin^2(pi e_k) / lambda_k)).
The seasonal term is locally_periodic_closed_form's.  k(x, x) = s_t + s_s; a non-finite difference gives NaN (the seasonal
term's).

``trend_seasonal_torch`` is a base-kernel callable for the CPU oracle (oracle.pls_oracle), ``trend_seasonal_numpy`` one for
oracle.selectors_oracle; ``trend_seasonal_factors_numpy`` gives both kappas and the derivative factors of pairs from their
differences, ``trend_sensitivity`` the first-order sensitivity of the trend's exponent to a relative error in the differences
(the seasonal term's is locally_periodic_closed_form.sensitivity)."""
import numpy as np
import torch

from locally_periodic_closed_form import LN2, locally_periodic_factors_numpy, locally_periodic_torch, sensitivity  # noqa: F401


def trend_seasonal_factors_numpy(delta, lengthscale, seasonal_lengthscale, periodic_lengthscale, period):
    """(kappa_t (...), ft (..., d), kappa_s (...), fe, fl, fp, e (..., d) each) of pairs with differences delta (..., d):
    ft_k = (delta_k / l_k)^2, d kappa_t / d log l_k = kappa_t ft_k, kappa_t = exp(-sum_k ft_k / 2); the rest as
    locally_periodic_factors_numpy gives it for (m, lambda, p)."""
    delta = np.asarray(delta, dtype=np.float64)
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        ft = np.square(delta / ls)
        kap_t = np.exp(-(0.5 * ft).sum(-1))
    return (kap_t, ft) + locally_periodic_factors_numpy(delta, seasonal_lengthscale, periodic_lengthscale, period)


def trend_sensitivity(delta, lengthscale):
    """c_t = 1 + r_t^2 with r_t^2 = sum_k (delta_k / l_k)^2: a relative error eps in every difference moves the trend's exponent
    r_t^2 / 2 by at most r_t^2 eps, and the 1 stands for the rounding of the exponential itself"""
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    return 1.0 + np.square(np.asarray(delta, dtype=np.float64) / ls).sum(-1)


def trend_seasonal_numpy(lengthscale, outputscale=1.0, seasonal_lengthscale=1.0, periodic_lengthscale=1.0, period=1.0,
                         seasonal_outputscale=1.0):
    def k(x1, x2):
        delta = np.asarray(x1, dtype=np.float64)[:, None, :] - np.asarray(x2, dtype=np.float64)[None, :, :]
        f = trend_seasonal_factors_numpy(delta, lengthscale, seasonal_lengthscale, periodic_lengthscale, period)
        return float(outputscale) * f[0] + float(seasonal_outputscale) * f[2]

    return k


def trend_seasonal_torch(lengthscale, outputscale=1.0, seasonal_lengthscale=1.0, periodic_lengthscale=1.0, period=1.0,
                         seasonal_outputscale=1.0):
    ls = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1)
    seasonal = locally_periodic_torch(seasonal_lengthscale, seasonal_outputscale, periodic_lengthscale, period)

    def k(x1, x2):
        x1 = x1 if x1.dim() == 2 else x1[:, None]
        x2 = x2 if x2.dim() == 2 else x2[:, None]
        delta = x1[:, None, :].double() - x2[None, :, :].double()
        return float(outputscale) * torch.exp(-0.5 * (delta / ls).square().sum(-1)) + seasonal(x1, x2)

    return k
