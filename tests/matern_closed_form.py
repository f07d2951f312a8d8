"""Closed forms of gpytorch's ScaleKernel(MaternKernel(nu)) with ARD lengthscales, the yardstick of the Matern tests.

r = |(a - b) / lengthscale| from direct differences (not gpytorch's |a|^2 + |b|^2 - 2 a.b, which loses accuracy near
r = 0, nor its mean-centring, which changes only the rounding), and with the outputscale s:
    nu = 1/2:  s * exp(-r)
    nu = 3/2:  s * (1 + sqrt3 r) * exp(-sqrt3 r)
    nu = 5/2:  s * (1 + sqrt5 r + 5 r^2 / 3) * exp(-sqrt5 r)
An entry whose exponential is 0 is 0 (r = inf included, where the polynomial alone would make it NaN).

``matern_torch`` is a base-kernel callable for the CPU oracle (oracle.pls_oracle), ``matern_numpy`` one for
oracle.selectors_oracle."""
import math

import numpy as np
import torch

NUS = (0.5, 1.5, 2.5)


def _value(r, nu, outputscale, exp, where):
    if nu == 0.5:
        e = exp(-r)
        k = e
    elif nu == 1.5:
        e = exp(-math.sqrt(3.0) * r)
        k = (1.0 + math.sqrt(3.0) * r) * e
    elif nu == 2.5:
        e = exp(-math.sqrt(5.0) * r)
        k = (1.0 + math.sqrt(5.0) * r + 5.0 * r * r / 3.0) * e
    else:
        raise ValueError(f"nu must be one of {NUS}, got {nu}")
    return outputscale * where(e == 0.0, 0.0, k)


def matern_torch(lengthscale, outputscale=1.0, nu=2.5):
    ls = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1)

    def k(x1, x2):
        x1 = x1 if x1.dim() == 2 else x1[:, None]
        x2 = x2 if x2.dim() == 2 else x2[:, None]
        diff = (x1[:, None, :].double() - x2[None, :, :].double()) / ls
        r = diff.square().sum(-1).sqrt()
        return _value(r, nu, float(outputscale), torch.exp, lambda c, a, b: torch.where(c, torch.zeros_like(b), b))

    return k


def matern_numpy(lengthscale, outputscale=1.0, nu=2.5):
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)

    def k(x1, x2):
        diff = (np.asarray(x1, dtype=np.float64)[:, None, :] - np.asarray(x2, dtype=np.float64)[None, :, :]) / ls
        r = np.sqrt((diff**2).sum(-1))
        with np.errstate(invalid="ignore", over="ignore"):
            return _value(r, nu, float(outputscale), np.exp, np.where)

    return k
