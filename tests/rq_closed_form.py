"""Closed form of gpytorch's ScaleKernel(RQKernel) with ARD lengthscales (as recalled; include/plship.h states the formula),
the yardstick of the rational-quadratic tests.

r^2 = sum_k ((a_k - b_k) / lengthscale_k)^2 from direct differences (not |a|^2 + |b|^2 - 2 a.b, which loses accuracy near
r = 0), u = r^2 / (2 alpha) and, with the outputscale s,
    k = s * (1 + u)^(-alpha) = s * exp(-alpha * log1p(u)),
through log1p, so that a small u keeps its digits and k(x, x) = s exactly.  r = inf gives 0.

``rq_torch`` is a base-kernel callable for the CPU oracle (oracle.pls_oracle), ``rq_numpy`` one for
oracle.selectors_oracle; ``rq_factors_numpy`` gives kappa and the two derivative factors of a pair from its r^2."""
import numpy as np
import torch

LN2 = 0.6931471805599453  # alpha at raw alpha = 0
ALPHAS = (0.05, LN2, 3.0, 1e3, 1e6)


def rq_torch(lengthscale, outputscale=1.0, alpha=1.0):
    ls = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1)
    alpha = float(alpha)

    def k(x1, x2):
        x1 = x1 if x1.dim() == 2 else x1[:, None]
        x2 = x2 if x2.dim() == 2 else x2[:, None]
        diff = (x1[:, None, :].double() - x2[None, :, :].double()) / ls
        r2 = diff.square().sum(-1)
        return float(outputscale) * torch.exp(-alpha * torch.log1p(r2 / (2.0 * alpha)))

    return k


def rq_numpy(lengthscale, outputscale=1.0, alpha=1.0):
    ls = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
    alpha = float(alpha)

    def k(x1, x2):
        diff = (np.asarray(x1, dtype=np.float64)[:, None, :] - np.asarray(x2, dtype=np.float64)[None, :, :]) / ls
        with np.errstate(over="ignore"):
            r2 = (diff**2).sum(-1)
            return float(outputscale) * np.exp(-alpha * np.log1p(r2 / (2.0 * alpha)))

    return k


def rq_factors_numpy(r2, alpha):
    """(kappa, g, ga) of pairs at squared scaled distance r2: kappa = (1 + u)^-alpha, g = kappa / (1 + u) (d kappa / d log l_k =
    g e_k^2) and ga = d kappa / d log alpha = alpha kappa (u / (1 + u) - log1p(u)).  The bracket is -u^2/2 + 2u^3/3 - ... for a
    small u, where its two terms cancel: below u = 0.1 it is summed from its series -sum_{m>=2} (-u)^m (m - 1) / m, which
    keeps full precision (60 terms: truncation below 1e-60)."""
    r2 = np.asarray(r2, dtype=np.float64)
    alpha = float(alpha)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        u = r2 / (2.0 * alpha)
        lg = np.log1p(u)
        kap = np.exp(-alpha * lg)
        g = np.where(np.isinf(u), 0.0, kap / (1.0 + u))
        direct = u / (1.0 + u) - lg
        series = np.zeros_like(u)
        small = np.where(u < 0.1, u, 0.0)
        for m in range(60, 1, -1):  # Horner in -u, coefficients -(m - 1) / m
            series = -(m - 1.0) / m + series * (-small)
        series = series * small * small
        h = np.where(u < 0.1, series, direct)
        ga = np.where(np.isinf(u), 0.0, alpha * kap * h)
    return kap, g, ga
