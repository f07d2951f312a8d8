"""Ordinal cost for ordered categories: the cumulative-logit (proportional-odds) model (not in the reference;
include/plship.h states the contract)."""
import math

import torch

from .. import _lib as L
from ..link_functions import PLSLinkFunction
from .base import PLSCost

MAX_CATEGORIES = 5  # the four p[] slots of the descriptor hold the cutpoints


def _checked_cutpoints(cutpoints) -> tuple:
    b = tuple(float(c) for c in (cutpoints.tolist() if isinstance(cutpoints, torch.Tensor) else cutpoints))
    if len(b) > MAX_CATEGORIES - 1:
        raise ValueError(f"OrdinalCost takes at most {MAX_CATEGORIES - 1} cutpoints: the limit is {MAX_CATEGORIES} categories, "
                         f"got {len(b) + 1}")
    if len(b) < 1:
        raise ValueError("OrdinalCost needs at least one cutpoint (two categories)")
    if not all(math.isfinite(c) for c in b):
        raise ValueError(f"OrdinalCost needs finite cutpoints, got {b}")
    if any(hi <= lo for lo, hi in zip(b, b[1:])):
        raise ValueError(f"OrdinalCost needs strictly increasing cutpoints, got {b}")
    return b


class OrdinalCost(PLSCost):
    """Categories 0 .. K-1 (2 <= K <= 5) with cutpoints b_1 < ... < b_(K-1), b_0 = -inf, b_K = +inf, and
    P(y <= k | f) = sigmoid(b_(k+1) - f).  For label k between lo = b_k and hi = b_(k+1),
    c_j = sum_n softplus(f_nj - hi_n) + softplus(lo_n - f_nj): the negative log-likelihood without its f-independent term
    -log(1 - exp(-(hi - lo))) (energies are comparable between runs with the same ``cutpoints`` only).  The derivative
    sigmoid(f - hi) - sigmoid(lo - f) lies in (-1, 1): a bounded drift.  The latent f enters directly (IdentityLinkFunction;
    the library refuses any other link).  With K = 2 and the cutpoint 0 this is the Bernoulli/sigmoid cost without its
    clip."""

    cost_kind = L.COST_ORDINAL

    def __init__(self, y_train: torch.Tensor, link_function: PLSLinkFunction, cutpoints):
        super().__init__(link_function=link_function, observation_noise=None)
        self.cutpoints = cutpoints
        k = self.number_of_categories
        y = y_train.detach().to(torch.float64)
        if y.numel() and not bool(((y == y.round()) & (y >= 0) & (y <= k - 1)).all()):
            raise ValueError(f"OrdinalCost needs every label to be an integer in [0, {k - 1}] ({k} categories)")
        self.y_train = y_train

    @property
    def cutpoints(self) -> tuple:
        """the finite cutpoints, ascending (assigning validates them)"""
        return self._cutpoints

    @cutpoints.setter
    def cutpoints(self, value) -> None:
        self._cutpoints = _checked_cutpoints(value)

    @property
    def number_of_categories(self) -> int:
        return len(self._cutpoints) + 1

    @staticmethod
    def cutpoints_from_labels(y: torch.Tensor, num_categories: int | None = None) -> list:
        """The logits of the smoothed empirical cumulative frequencies (half an observation added to every category), so
        that a latent at 0 reproduces the marginal frequencies.  Host arithmetic on K numbers."""
        labels = y.detach().reshape(-1).cpu().to(torch.float64)
        if not bool(((labels == labels.round()) & (labels >= 0)).all()):
            raise ValueError("cutpoints_from_labels needs non-negative integer labels")
        k = int(labels.max().item()) + 1 if num_categories is None else int(num_categories)
        if not 2 <= k <= MAX_CATEGORIES or (labels.numel() and int(labels.max().item()) > k - 1):
            raise ValueError(f"cutpoints_from_labels needs 2 to {MAX_CATEGORIES} categories that hold every label, got {k}")
        counts = torch.bincount(labels.to(torch.long), minlength=k).to(torch.float64) + 0.5
        cum = torch.cumsum(counts, 0)[:-1] / counts.sum()
        return (torch.log(cum) - torch.log1p(-cum)).tolist()

    def _params(self) -> tuple:
        return self._cutpoints + (math.inf,) * (MAX_CATEGORIES - 1 - len(self._cutpoints))

    def category_probabilities(self, f: torch.Tensor) -> torch.Tensor:
        """(...,) -> (..., K): P(y = k | f) = sigmoid(hi - f) sigmoid(f - lo) (1 - exp(-(hi - lo))) -- a product, not a
        difference of two numbers near 1; an edge category is the one sigmoid."""
        b = torch.tensor(self._cutpoints, dtype=f.dtype, device=f.device)
        t = f[..., None] - b  # (..., K - 1)
        below, above = torch.sigmoid(-t), torch.sigmoid(t)  # P(y <= k), P(y > k) for k = 0 .. K-2
        width = -torch.expm1(-(b[1:] - b[:-1]))
        inner = below[..., 1:] * above[..., :-1] * width
        return torch.cat([below[..., :1], inner, above[..., -1:]], dim=-1)

    def predict(self, prediction_samples: torch.Tensor) -> torch.distributions.Categorical:
        """(n, J) latent samples -> Categorical over the K categories per test point, the probabilities averaged over the
        particles"""
        return torch.distributions.Categorical(probs=self.category_probabilities(prediction_samples).mean(dim=1))
