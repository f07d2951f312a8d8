"""The metrics the step-size search optimises (drop-in for experiments/metrics.py:23-146, the branches that apply to
PLS and conformal predictions).  Inputs are per-test-point vectors: host-side arithmetic on N* numbers."""
from __future__ import annotations

import math

import torch

from .conformalise import ConformalPrediction


def _point(prediction) -> torch.Tensor:
    if isinstance(prediction, torch.distributions.MultivariateNormal):
        return prediction.mean
    if isinstance(prediction, torch.distributions.Bernoulli):
        return prediction.probs
    if isinstance(prediction, torch.distributions.Poisson):
        return prediction.rate
    if isinstance(prediction, torch.distributions.StudentT):
        return prediction.loc
    if isinstance(prediction, (torch.distributions.NegativeBinomial, torch.distributions.Beta, torch.distributions.Gamma)):  # (not in the reference)
        return prediction.mean
    if isinstance(prediction, torch.distributions.Categorical):  # (not in the reference) the expected category index
        return prediction.probs @ torch.arange(prediction.probs.shape[-1], dtype=prediction.probs.dtype, device=prediction.probs.device)
    if isinstance(prediction, ConformalPrediction):
        return prediction.mean
    raise ValueError(f"Prediction type {type(prediction)} not supported")


def calculate_mae(prediction, y: torch.Tensor) -> float:
    p = _point(prediction)
    return p.sub(y.to(p)).abs().mean().item()  # metrics.py:23-45


def calculate_mse(prediction, y: torch.Tensor) -> float:
    p = _point(prediction)
    return p.sub(y.to(p)).pow(2).mean().item()  # metrics.py:48-70


def calculate_nll(prediction, y: torch.Tensor) -> float:
    """metrics.py:73-125."""
    if isinstance(prediction, torch.distributions.MultivariateNormal):
        # gpytorch.metrics.mean_standardized_log_loss without train_y: mean 0.5 (log(2 pi s^2) + (y - m)^2 / s^2)
        m, v = prediction.mean, torch.diagonal(prediction.covariance_matrix)
        yy = y.to(m)
        return (0.5 * (torch.log(2 * math.pi * v) + torch.square(yy - m) / v)).mean().item()
    if isinstance(prediction, torch.distributions.Bernoulli):
        return torch.nn.functional.binary_cross_entropy(prediction.probs, y.to(prediction.probs), reduction="mean").item()
    if isinstance(prediction, torch.distributions.Poisson):
        return torch.nn.functional.poisson_nll_loss(prediction.rate, y.to(prediction.rate), reduction="mean").item()
    if isinstance(prediction, torch.distributions.StudentT):
        return prediction.log_prob(y.to(prediction.loc)).mean().item()  # metrics.py:98-99 (sign as in the reference)
    if isinstance(prediction, (torch.distributions.NegativeBinomial, torch.distributions.Beta, torch.distributions.Gamma)):  # (not in the reference)
        return -prediction.log_prob(y.to(prediction.mean)).mean().item()
    if isinstance(prediction, torch.distributions.Categorical):  # (not in the reference)
        return -prediction.log_prob(y.to(device=prediction.probs.device, dtype=torch.long)).mean().item()
    if isinstance(prediction, ConformalPrediction):
        # metrics.py:100-117: half the width of the 2/3 interval as the standard deviation of a normal around the median
        assert prediction.coverage == 2 / 3, f"NLL calculation needs 2/3 coverage, got {prediction.coverage=}"
        std = ((prediction.upper - prediction.lower) / 2).to(torch.float64)
        z = (y.to(std) - prediction.mean.to(std)) / std
        return (0.5 * z.square() + torch.log(std) + 0.5 * math.log(2 * math.pi)).mean().item()
    raise ValueError(f"Prediction type {type(prediction)} not supported")


def calculate_coverage(prediction: ConformalPrediction, y: torch.Tensor) -> float:
    """metrics.py:122-126: the share of targets inside [lower, upper] (a float32 mean, as the reference's ``.float()``)."""
    yy = y.to(prediction.lower)
    return ((prediction.lower <= yy) & (yy <= prediction.upper)).float().mean().item()


def calculate_average_interval_width(model, x: torch.Tensor, coverage: float) -> float:
    """metrics.py:129-137: ``model`` is a ConformalisePLS or a ConformaliseGP."""
    return model.calculate_average_interval_width(x=x, coverage=coverage)


def calculate_median_interval_width(model, x: torch.Tensor, coverage: float) -> float:
    """metrics.py:140-146."""
    lower, upper = model.predict_coverage(x=x, coverage=coverage)
    return torch.median(upper - lower).item()
