"""Negative-binomial cost for over-dispersed counts (not in the reference; include/plship.h states the contract)."""
import torch

from .. import _lib as L
from ..link_functions import PLSLinkFunction
from .base import PLSCost


class NegativeBinomialCost(PLSCost):
    """c_j = sum_n r log1p(mu_nj / r) + y_n log1p(r / mu_nj), mu = link(f): the negative log-likelihood of a negative binomial
    with mean mu and variance mu + mu^2 / r, without its f-independent terms (energies are comparable between runs with the
    same ``dispersion`` only).  With ExponentialLinkFunction the library evaluates it in t = f - log r as
    r softplus(t) + y softplus(-t), derivative r sigmoid(t) - y sigmoid(-t) in [-y, r]; a large r approaches the Poisson
    drift mu - y of a log link."""

    cost_kind = L.COST_NEGATIVE_BINOMIAL

    def __init__(self, y_train: torch.Tensor, link_function: PLSLinkFunction, dispersion: float):
        super().__init__(link_function=link_function, observation_noise=None)
        self.y_train = y_train
        self.dispersion = float(dispersion)  # (validated by the library with every call: finite and > 0)

    def _params(self) -> tuple:
        return (self.dispersion, 0.0, 0.0, 0.0)

    def predict(self, prediction_samples: torch.Tensor) -> torch.distributions.NegativeBinomial:
        mu = prediction_samples.mean(dim=1)
        r = torch.as_tensor(self.dispersion, dtype=mu.dtype, device=mu.device)
        return torch.distributions.NegativeBinomial(total_count=r, probs=mu / (r + mu))
