"""The likelihood objects of the SVGP baseline, as the reference's drivers pass them to ``SVGP(..., likelihood=...)``:
plain holders of what the library's per-point epilogue needs (include/plship.h, "SVGP with a quadrature likelihood").
No gpytorch objects anywhere."""
from __future__ import annotations

import math

from . import _lib as L


class _Likelihood:
    code: int = L.SVGP_GAUSSIAN
    #: the floor under the noise: noise = softplus(raw) + noise_floor; None for a likelihood without a noise
    noise_floor: float | None = 0.0
    deg_free: float = 0.0
    noise: float | None = None

    def _start_noise(self, noise):
        if noise is not None and not float(noise) > self.noise_floor:
            raise ValueError(f"{type(self).__name__}: the noise must exceed {self.noise_floor}")
        return None if noise is None else float(noise)


class GaussianLikelihood(_Likelihood):
    """gpytorch's GaussianLikelihood: noise = softplus(raw) + 1e-4 (GreaterThan(1e-4)).  ``noise``: the starting value
    (raw value 0 when None).  The closed-form epilogue: the path of ``likelihood="gaussian"``."""
    code, noise_floor = L.SVGP_GAUSSIAN, 1e-4

    def __init__(self, noise: float | None = None):
        self.noise = self._start_noise(noise)


class BernoulliLikelihood(_Likelihood):
    """gpytorch's BernoulliLikelihood: p(y = 1 | f) = Phi(f), labels in {0, 1}; 20-node Gauss-Hermite quadrature.  It has
    no parameter."""
    code, noise_floor = L.SVGP_BERNOULLI, None


class StudentTLikelihood(_Likelihood):
    """gpytorch's StudentTLikelihood with the degrees of freedom FIXED (the reference pins them inside an interval of
    width 2e-10): scale^2 = noise = softplus(raw), no floor (Positive).  ``noise``: the starting value (raw value 0 when
    None); 20-node Gauss-Hermite quadrature."""
    code, noise_floor = L.SVGP_STUDENT_T, 0.0

    def __init__(self, deg_free: float, noise: float | None = None):
        self.deg_free = float(deg_free)
        if not (math.isfinite(self.deg_free) and self.deg_free > 2.0):
            raise ValueError(f"StudentTLikelihood: deg_free must be finite and > 2, got {deg_free}")
        self.noise = self._start_noise(noise)
