"""Gamma cost for strictly positive, right-skewed continuous data under the log link (not in the reference;
include/plship.h states the contract)."""
import math

import torch

from .. import _lib as L
from ..kernel import _dev
from ..link_functions import PLSLinkFunction
from .base import PLSCost


def _checked_concentration(value) -> float:
    k = float(value)
    if not (k > 0 and math.isfinite(k)):
        raise ValueError(f"GammaCost needs a finite concentration (shape) > 0, got {k}")
    return k


class GammaCost(PLSCost):
    """c_j = sum_n k (exp(t_nj) - t_nj) with t = log y_n - f_nj: the negative log-likelihood of a Gamma distribution with shape
    ``concentration`` = k and mean mu = exp(f) (variance mu^2 / k), without its f-independent terms (energies are comparable
    between runs with the same ``concentration`` only).  The library receives z = log y, converted once here, and evaluates
    value and derivative -k expm1(t) in t; the derivative is bounded above by k but not below, and its slope is k e^t: the
    stable step size behaves like PoissonCost's, not like that of the bounded families.  The mean enters as exp(f)
    (ExponentialLinkFunction; the library refuses any other link)."""

    cost_kind = L.COST_GAMMA

    def __init__(self, y_train: torch.Tensor, link_function: PLSLinkFunction, concentration: float):
        super().__init__(link_function=link_function, observation_noise=None)
        if getattr(link_function, "kind", None) != L.LINK_EXP:
            raise ValueError(f"GammaCost needs ExponentialLinkFunction (the log link), got {type(link_function).__name__}")
        if not bool((torch.isfinite(y_train) & (y_train > 0)).all()):
            raise ValueError("GammaCost needs every y finite and > 0")
        self.y_train = y_train
        self.concentration = concentration
        self._z_dev = None

    @property
    def concentration(self) -> float:
        """the shape k (assigning validates it)"""
        return self._concentration

    @concentration.setter
    def concentration(self, value) -> None:
        self._concentration = _checked_concentration(value)

    @classmethod
    def from_logs(cls, log_y: torch.Tensor, link_function: PLSLinkFunction, concentration: float) -> "GammaCost":
        """For observations held as z = log y (any finite z: observations beyond the fp64 range of y); ``y_train`` becomes
        exp(z), kept inside the positive fp64 range."""
        if not bool(torch.isfinite(log_y).all()):
            raise ValueError("GammaCost.from_logs needs finite logarithms")
        z = log_y.to(torch.float64)
        y = torch.exp(z).clamp(5e-324, torch.finfo(torch.float64).max)
        cost = cls(y, link_function, concentration)
        cost._z_dev, cost._z_src = _dev(z.reshape(-1)), y
        return cost

    def y_device(self) -> torch.Tensor:
        """the library's y argument: the fp64 logarithm of y_train, cached"""
        y = self.y_train
        if self._z_dev is None or self._z_src is not y:
            self._z_dev = _dev(torch.log(y.detach().to(torch.float64).reshape(-1)))
            self._z_src = y
        return self._z_dev

    def _params(self) -> tuple:
        return (self._concentration, 0.0, 0.0, 0.0)

    @staticmethod
    def estimate_concentration(y: torch.Tensor, mean: torch.Tensor) -> float:
        """The maximum-likelihood shape for given means: the root of log k - psi(k) = s, s = mean(y / mu - log(y / mu) - 1)
        (> 0 unless every y equals its mean).  Newton in log k from the closed-form start
        k = (3 - s + sqrt((s - 3)^2 + 24 s)) / (12 s); host arithmetic on one number."""
        y64 = y.detach().reshape(-1).cpu().to(torch.float64)
        mu = torch.as_tensor(mean).detach().reshape(-1).cpu().to(torch.float64)
        mu = mu.expand_as(y64) if mu.numel() == 1 else mu  # (one mean for all: a constant model)
        if y64.numel() == 0 or y64.shape != mu.shape:
            raise ValueError("estimate_concentration needs as many means as observations, and at least one")
        if not bool((torch.isfinite(y64) & (y64 > 0) & torch.isfinite(mu) & (mu > 0)).all()):
            raise ValueError("estimate_concentration needs every y and every mean finite and > 0")
        ratio = y64 / mu
        s = float((ratio - torch.log(ratio) - 1).mean())
        if not s > 0:
            raise ValueError("estimate_concentration: s = mean(y / mu - log(y / mu) - 1) is not positive -- every y equals its "
                             "mean, and the likelihood has no maximum in the shape")
        return GammaCost._solve_concentration(s)

    @staticmethod
    def _solve_concentration(s: float) -> float:
        """the root k of log k - psi(k) = s for s > 0"""
        u = torch.tensor(math.log((3 - s + math.sqrt((s - 3) ** 2 + 24 * s)) / (12 * s)), dtype=torch.float64)
        for _ in range(50):
            k = torch.exp(u)
            g = u - torch.digamma(k) - s
            step = g / (1 - k * torch.polygamma(1, k))  # (k psi'(k) > 1: the slope is negative everywhere)
            u = u - step
            if abs(float(step)) <= 2.0 ** -52 * max(1.0, abs(float(u))):
                break
        return float(torch.exp(u))

    def predict(self, prediction_samples: torch.Tensor) -> torch.distributions.Gamma:
        """(n, J) link values -> Gamma(concentration=k, rate=k / mu) per test point, mu the particle mean"""
        mu = prediction_samples.mean(dim=1)
        k = torch.as_tensor(self._concentration, dtype=mu.dtype, device=mu.device)
        return torch.distributions.Gamma(concentration=k.expand_as(mu), rate=k / mu)
