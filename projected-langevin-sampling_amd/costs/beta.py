"""Beta cost for proportions in (0, 1) (not in the reference; include/plship.h states the contract)."""
import torch

from .. import _lib as L
from ..kernel import _dev
from ..link_functions import PLSLinkFunction
from .base import PLSCost


class BetaCost(PLSCost):
    """c_j = sum_n lgamma(a_nj) + lgamma(b_nj) - a_nj z_n with a = phi mu, b = phi (1 - mu), mu = link(f) and
    z_n = logit(y_n): the negative log-likelihood of a Beta distribution with mean mu and precision phi (variance
    mu (1 - mu) / (1 + phi)), without its f-independent terms (energies are comparable between runs with the same
    ``precision`` only).  The library receives the logits z, converted once here; with SigmoidLinkFunction it evaluates the
    pair in f without the link's clip, and the derivative tends to +-1 as f -> +-inf: a bounded drift."""

    cost_kind = L.COST_BETA

    def __init__(self, y_train: torch.Tensor, link_function: PLSLinkFunction, precision: float):
        super().__init__(link_function=link_function, observation_noise=None)
        if not bool(((y_train > 0) & (y_train < 1)).all()):
            raise ValueError("BetaCost needs every y strictly inside (0, 1)")
        self.y_train = y_train
        self.precision = float(precision)  # (validated by the library with every call: finite and > 0)
        self._z_dev = None

    @classmethod
    def from_logits(cls, z_train: torch.Tensor, link_function: PLSLinkFunction, precision: float) -> "BetaCost":
        """For observations held as logits z = log y - log1p(-y) (any finite z: proportions nearer to 0 or 1 than fp64 can
        hold them); ``y_train`` becomes sigmoid(z)."""
        if not bool(torch.isfinite(z_train).all()):
            raise ValueError("BetaCost.from_logits needs finite logits")
        z = z_train.to(torch.float64)
        y = torch.sigmoid(z).clamp(5e-324, 1 - 2.0 ** -53)
        cost = cls(y, link_function, precision)
        cost._z_dev, cost._z_src = _dev(z.reshape(-1)), y
        return cost

    def y_device(self) -> torch.Tensor:
        """the library's y argument: the fp64 logit of y_train, cached"""
        y = self.y_train
        if self._z_dev is None or self._z_src is not y:
            y64 = y.detach().to(torch.float64).reshape(-1)
            self._z_dev = _dev(torch.log(y64) - torch.log1p(-y64))
            self._z_src = y
        return self._z_dev

    def _params(self) -> tuple:
        return (self.precision, 0.0, 0.0, 0.0)

    def predict(self, prediction_samples: torch.Tensor) -> torch.distributions.Beta:
        mu = prediction_samples.mean(dim=1)
        return torch.distributions.Beta(mu * self.precision, (1 - mu) * self.precision)
