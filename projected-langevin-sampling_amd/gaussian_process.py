"""Exact-GP hyper-parameters on the device: the second stage of every experiment of the reference (data, exact-GP
hyper-parameters, inducing points, PLS, metrics).

Replaces ``src/gaussian_process/exact_gp.py`` as it is used by ``train_exact_gp`` (experiments/trainers.py:15-52),
``exact_gp_runner`` / ``load_subsample_data`` (experiments/runners.py:66-187) and the two averaging constructors
(experiments/constructors.py:9-53).  The reference builds these on gpytorch (ConstantMean, ScaleKernel(RBFKernel |
MaternKernel), GaussianLikelihood, ExactMarginalLogLikelihood); here the model is a plain parameter holder and one
evaluation of the marginal log-likelihood with its gradient is ONE library call, ``pls_gp_mll_grad`` (csrc/gp_mll.hip).
One output, Gaussian likelihood; no gpytorch objects anywhere."""
from __future__ import annotations

import math
import warnings
from typing import Callable, List, Sequence, Tuple

import torch

from . import _lib as L
from ._chol import CHOLESKY_JITTER, CHOLESKY_MAX_TRIES, NotPSDError, cholesky_factor
from .kernel import ARDKernel, BaseKernel, MaternKernel
from .trainers import EarlyStopper
from .utils import set_seed

#: gpytorch's GaussianLikelihood keeps its noise above this bound (GreaterThan(1e-4)): noise = 1e-4 + softplus(raw)
NOISE_LOWER_BOUND = 1e-4

_KERNEL_NAMES = {"rbf": ("rbf", None), "matern": ("matern", None), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5),
                 "matern52": ("matern", 2.5)}


def _softplus(v: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.softplus(v)


def _inverse_softplus(v: torch.Tensor) -> torch.Tensor:
    return v + torch.log(-torch.expm1(-v))


class ExactGP:
    """Exact GP regression with a constant mean, a scaled stationary kernel and Gaussian noise, parametrised as gpytorch
    does: ``lengthscale = softplus(raw)``, ``outputscale = softplus(raw)``, ``noise = 1e-4 + softplus(raw)``, the mean
    constant itself; every raw value starts at 0.

    ``raw`` is ONE float64 CPU tensor, in this order::

        raw[0]   the mean constant
        raw[1]   raw noise
        raw[2]   raw outputscale
        raw[3:]  raw lengthscales: d of them (``ard=True``) or one shared by all dimensions (``ard=False``)

    ``kernel``: "rbf" or "matern" (with ``nu``); "matern12" / "matern32" / "matern52" name nu as well; an ARDKernel /
    MaternKernel instance gives the kind and the starting values (as the reference's ``deepcopy(kernel)``).
    x (n, d) and y (n) are kept as given and uploaded once, on the first evaluation on the device."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, kernel="rbf", nu: float = 2.5, ard: bool = True):
        x = x.detach()
        self.x = (x if x.dim() == 2 else x[:, None]).to(torch.float64)
        self.y = y.detach().reshape(-1).to(torch.float64)
        assert self.x.shape[0] == self.y.shape[0] and self.x.shape[0] > 0, "x (n, d) and y (n) must share n > 0"
        self.n, self.d = self.x.shape
        start = None
        if isinstance(kernel, BaseKernel):
            if not isinstance(kernel, (ARDKernel, MaternKernel)):
                raise TypeError("ExactGP: the kernel must be an ARDKernel or a MaternKernel (a lengthscale and an outputscale to learn)")
            start = kernel
            name, nu = ("matern", kernel.nu) if isinstance(kernel, MaternKernel) else ("rbf", nu)
            ard = kernel.lengthscale.numel() > 1 or self.d == 1 and ard
        else:
            if kernel not in _KERNEL_NAMES:
                raise ValueError(f"ExactGP: kernel must be one of {sorted(_KERNEL_NAMES)} or a kernel object, got {kernel!r}")
            name, named_nu = _KERNEL_NAMES[kernel]
            nu = named_nu if named_nu is not None else nu
        self.kernel_name, self.ard = name, bool(ard)
        self.nu = float(nu) if name == "matern" else None
        if name == "matern" and self.nu not in MaternKernel.KINDS:
            raise ValueError(f"ExactGP: nu must be 0.5, 1.5 or 2.5, got {nu}")
        self.kind = MaternKernel.KINDS[self.nu] if name == "matern" else L.KERNEL_RBF_ARD
        nls = self.d if self.ard else 1
        raw = torch.zeros(3 + nls, dtype=torch.float64)
        if start is not None:
            assert start.lengthscale.numel() in (1, nls), "the kernel's lengthscales do not fit the data"
            raw[2] = _inverse_softplus(torch.tensor(start.outputscale, dtype=torch.float64))
            raw[3:] = _inverse_softplus(start.lengthscale.expand(nls) if start.lengthscale.numel() == 1 else start.lengthscale)
        self.raw = torch.nn.Parameter(raw)
        self._dev: dict = {}

    # ---- parameters -------------------------------------------------------------------------------------------------
    def raw_parameters(self) -> torch.Tensor:
        """A copy of ``raw`` (float64, CPU; the order is in the class docstring)."""
        return self.raw.detach().clone()

    def set_raw_parameters(self, raw: torch.Tensor) -> "ExactGP":
        raw = torch.as_tensor(raw, dtype=torch.float64).reshape(-1)
        assert raw.numel() == self.raw.numel(), f"{self.raw.numel()} raw parameters expected, got {raw.numel()}"
        with torch.no_grad():
            self.raw.copy_(raw)
        return self

    @property
    def mean_constant(self) -> float:
        return float(self.raw.detach()[0])

    @property
    def noise(self) -> float:
        return NOISE_LOWER_BOUND + float(_softplus(self.raw.detach()[1]))

    @property
    def outputscale(self) -> float:
        return float(_softplus(self.raw.detach()[2]))

    @property
    def lengthscale(self) -> torch.Tensor:
        """d lengthscales (a shared one repeated)."""
        ls = _softplus(self.raw.detach()[3:])
        return ls.expand(self.d).clone() if ls.numel() == 1 and self.d > 1 else ls

    @property
    def kernel(self) -> BaseKernel:
        """The fitted base kernel: goes straight into PLSKernel and the inducing-point selectors."""
        if self.kernel_name == "matern":
            return MaternKernel(self.lengthscale, self.outputscale, nu=self.nu)
        return ARDKernel(self.lengthscale, self.outputscale)

    # ---- the loss ---------------------------------------------------------------------------------------------------
    def chain_rule(self, out: torch.Tensor) -> Tuple[float, torch.Tensor]:
        """(-mll / n, d(-mll / n) / d raw) from the 4 + d outputs of pls_gp_mll_grad (value, d/d mean, d/d noise,
        d/d log outputscale, d/d log lengthscale_k) at the current parameters: host arithmetic only."""
        out = torch.as_tensor(out, dtype=torch.float64).reshape(-1)
        assert out.numel() == 4 + self.d
        raw = self.raw.detach()
        slope = torch.sigmoid(raw)  # d softplus(raw) / d raw
        g = torch.empty_like(raw)
        g[0] = out[1]
        g[1] = out[2] * slope[1]
        g[2] = out[3] / _softplus(raw[2]) * slope[2]
        per_dim = out[4:] / self.lengthscale
        g[3:] = (per_dim if self.ard else per_dim.sum().reshape(1)) * slope[3:]
        return -float(out[0]) / self.n, -g / self.n

    def _device_state(self) -> dict:
        if not self._dev:
            from .kernel import _dev

            lib = L.load()
            x, y = _dev(self.x), _dev(self.y)
            nbytes = int(lib.pls_gp_mll_workspace_bytes(self.n, self.d))
            self._dev = {
                "x": x, "y": y,
                "ws": torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device),
                # the 4 + d outputs and, in the last slot, the int32 info word: one read-back per evaluation
                "out": torch.zeros(4 + self.d + 1, dtype=torch.float64, device=x.device),
            }
        return self._dev

    def evaluate_on_device(self, jitter: float = 0.0) -> Tuple[torch.Tensor, int]:
        """One pls_gp_mll_grad call at the current parameters: (the 4 + d outputs on the CPU, info)."""
        st = self._device_state()
        ls = st["x"].new_tensor(self.lengthscale.tolist())
        out, ws = st["out"], st["ws"]
        L.check(
            L.load().pls_gp_mll_grad(self.kind, st["x"].data_ptr(), self.n, self.d, ls.data_ptr(), self.outputscale, self.noise,
                                     self.mean_constant, float(jitter), st["y"].data_ptr(), out.data_ptr(),
                                     out.data_ptr() + 8 * (4 + self.d), ws.data_ptr(), ws.numel() * 8, L.stream_ptr()),
            "pls_gp_mll_grad",
        )
        host = out.cpu()
        return host[: 4 + self.d], int(host[4 + self.d:].view(torch.int32)[0])

    def loss_and_grad(self) -> Tuple[float, torch.Tensor]:
        """(-mll / n, its gradient with respect to ``raw``): gpytorch's ``-mll(model(x), y)`` and ``backward()``.  A
        factorisation that meets a non-positive pivot is retried with psd_safe_cholesky's jitters (1e-8, 1e-7, 1e-6), a
        warning per attempt, NotPSDError after the last."""
        attempts = [0.0] + [CHOLESKY_JITTER * 10**i for i in range(CHOLESKY_MAX_TRIES)]
        for jit in attempts:
            if jit > 0.0:
                warnings.warn(f"A not p.d., added jitter of {jit:.1e} to the diagonal", RuntimeWarning, stacklevel=2)
            out, info = self.evaluate_on_device(jit)
            if info == 0:
                return self.chain_rule(out)
        raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {attempts[-1]:.1e}.")

    # ---- prediction -------------------------------------------------------------------------------------------------
    def predict(self, x_test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(mean, latent variance, observation variance) at x_test (t, d), float64 on the device:
        c + k*^T alpha,  k** - |Lc^-1 k*|^2  and that plus the noise, with K_y = Lc Lc^T and alpha = K_y^-1 (y - c)."""
        st = self._device_state()
        kern = self.kernel
        ky = kern(st["x"], st["x"])
        ky.diagonal().add_(self.noise)
        factor = cholesky_factor(ky)
        alpha = factor.solve((st["y"] - self.mean_constant)[:, None])
        ks = kern(st["x"], x_test if x_test.dim() == 2 else x_test[:, None])  # (n, t): k-major
        t = ks.shape[1]
        mean = torch.empty((t, 1), dtype=torch.float64, device=ks.device)
        L.check(L.load().pls_gemm_tn(ks.data_ptr(), L.ld(ks), alpha.data_ptr(), 1, mean.data_ptr(), 1, t, 1, self.n, 1.0, 0.0,
                                     L.stream_ptr()), "pls_gemm_tn")
        v = factor.forward_solve(ks)
        var = self.outputscale - v.square().sum(dim=0)
        return mean[:, 0] + self.mean_constant, var, var + self.noise


def train_exact_gp(x: torch.Tensor, y: torch.Tensor, kernel, seed: int, number_of_epochs: int, learning_rate: float,
                   early_stopper_patience: float, evaluate: Callable[[ExactGP], Tuple[float, torch.Tensor]] | None = None,
                   ) -> Tuple[ExactGP, List[float]]:
    """experiments/trainers.py:15-52, statement for statement: seed, Adam over the raw parameters, and per epoch the
    loss, the early-stopper check BEFORE the loss is recorded and before the step, then the step.  ``evaluate(model) ->
    (loss, gradient)`` replaces ``model.loss_and_grad`` (a host evaluation drives the same loop without a device)."""
    set_seed(seed)
    model = ExactGP(x, y, kernel)
    evaluate = evaluate if evaluate is not None else ExactGP.loss_and_grad
    optimizer = torch.optim.Adam([model.raw], lr=learning_rate)
    losses: List[float] = []
    early_stopper = EarlyStopper(patience=early_stopper_patience)
    for _ in range(number_of_epochs):
        optimizer.zero_grad()
        loss, grad = evaluate(model)
        loss = float(loss)
        if early_stopper.should_stop(loss=loss, step_size=learning_rate):
            break
        losses.append(loss)
        model.raw.grad = torch.as_tensor(grad, dtype=torch.float64).reshape(model.raw.shape).clone()
        optimizer.step()
    return model, losses


def construct_average_ard_kernel(models: Sequence[ExactGP]) -> BaseKernel:
    """The kernel of the AVERAGED RAW parameters, softplus applied afterwards (constructors.py:28-53 averages the
    entries of ``state_dict()``, which are the raw values)."""
    first = models[0]
    raw = torch.stack([m.raw_parameters()[2:] for m in models]).mean(dim=0)
    outputscale, ls = float(_softplus(raw[0])), _softplus(raw[1:])
    ls = ls.expand(first.d).clone() if ls.numel() == 1 and first.d > 1 else ls
    if first.kernel_name == "matern":
        return MaternKernel(ls, outputscale, nu=first.nu)
    return ARDKernel(ls, outputscale)


def construct_average_gaussian_noise(models: Sequence[ExactGP]) -> float:
    """The mean of the noises themselves (constructors.py:9-25): the ``observation_noise`` of GaussianCost."""
    return float(torch.tensor([m.noise for m in models], dtype=torch.float64).mean())


def nearest_subsample(x: torch.Tensor, y: torch.Tensor, size: int, centre: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The ``size`` points of x nearest to ``centre`` (Euclidean), nearest first, and their targets: load_subsample_data
    (runners.py:66-85) without scikit-learn.  All of the data when ``size`` exceeds it."""
    if size > x.shape[0]:
        return x, y
    pts = x if x.dim() == 2 else x[:, None]
    dist = (pts - centre.reshape(1, -1).to(pts)).square().sum(dim=1)
    idx = torch.topk(dist, size, largest=False, sorted=True).indices
    return x[idx], y[..., idx]


def exact_gp_runner(x: torch.Tensor, y: torch.Tensor, kernel, subsample_size: int, seed: int, number_of_epochs: int,
                    learning_rate: float, number_of_iterations: int, early_stopper_patience: float) -> List[ExactGP]:
    """runners.py:88-187 without its files and plots: ``number_of_iterations`` exact GPs, each on the ``subsample_size``
    neighbours of a point drawn under ``seed + i``; ONE on all of the data when the subsample covers it."""
    if subsample_size >= x.shape[0]:
        number_of_iterations = 1
    models = []
    for i in range(number_of_iterations):
        set_seed(seed + i)
        centre = x[torch.randperm(x.shape[0])[0]]  # sample_point (src/samplers.py:47-62)
        xs, ys = nearest_subsample(x, y, subsample_size, centre)
        model, _ = train_exact_gp(xs, ys, kernel, seed, number_of_epochs, learning_rate, early_stopper_patience)
        models.append(model)
    return models


__all__ = ["ExactGP", "train_exact_gp", "construct_average_ard_kernel", "construct_average_gaussian_noise", "nearest_subsample",
           "exact_gp_runner", "NotPSDError"]
