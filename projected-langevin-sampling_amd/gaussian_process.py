"""Exact-GP hyper-parameters on the device: the second stage of every experiment of the reference (data, exact-GP
hyper-parameters, inducing points, PLS, metrics).

Replaces ``src/gaussian_process/exact_gp.py`` as it is used by ``train_exact_gp`` (experiments/trainers.py:15-52),
``exact_gp_runner`` / ``load_subsample_data`` (experiments/runners.py:66-187) and the two averaging constructors
(experiments/constructors.py:9-53).  The reference builds these on gpytorch (ConstantMean, ScaleKernel(RBFKernel |
MaternKernel | RQKernel | PeriodicKernel), GaussianLikelihood, ExactMarginalLogLikelihood); here the model is a plain parameter holder and one
evaluation of the marginal log-likelihood with its gradient is ONE library call, ``pls_gp_mll_grad_classes``
(csrc/gp_mll.hip; its pairwise kernels: csrc/base_kernel.hip).  One output with a Gaussian likelihood (``ExactGP``: one
class, no fixed noise), or classification with the Dirichlet likelihood of Milios et al. 2018 as the reference's two classification drivers use it (``DirichletExactGP``: one
GP per class); both are one private base class; no gpytorch objects anywhere."""
from __future__ import annotations

import ctypes
import math
import warnings
from typing import Callable, List, Sequence, Tuple

import torch

from . import _lib as L
from . import _ops
from ._chol import CHOLESKY_JITTER, CHOLESKY_MAX_TRIES, NotPSDError, cholesky_factor
from .kernel import STATIONARY_KERNELS, BaseKernel, LocallyPeriodicKernel, MaternKernel, PeriodicKernel, TrendSeasonalKernel, _dev
from .likelihoods import GaussianLikelihood, _Likelihood
from .trainers import EarlyStopper
from .utils import set_seed

#: gpytorch's GaussianLikelihood keeps its noise above this bound (GreaterThan(1e-4)): noise = 1e-4 + softplus(raw)
NOISE_LOWER_BOUND = 1e-4

#: the name table: what ``kernel`` may be as a string -> (the family of a class of kernel.STATIONARY_KERNELS, the nu it names).
#: A kernel CLASS names its family too, every raw value at 0.  It is the only way to ask the model classes for the periodic
#: family without starting values: they keep refusing the bare name "periodic" (train_exact_gp and exact_gp_runner take it)
_KERNEL_NAMES = {"rbf": ("rbf", None), "matern": ("matern", None), "matern12": ("matern", 0.5), "matern32": ("matern", 1.5),
                 "matern52": ("matern", 2.5), "rq": ("rq", None)}
#: the names that train_exact_gp and exact_gp_runner take beyond those: the families that the model classes take as a class
_TRAINER_KERNEL_NAMES = {"periodic": PeriodicKernel, "locally_periodic": LocallyPeriodicKernel, "trend_seasonal": TrendSeasonalKernel}
_FAMILIES = {cls.family: cls for cls in STATIONARY_KERNELS}


def _softplus(v: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.softplus(v)


def _inverse_softplus(v: torch.Tensor) -> torch.Tensor:
    return v + torch.log(-torch.expm1(-v))


def _repeated(v: torch.Tensor, width: int) -> torch.Tensor:
    """``v`` with ``width`` entries along its last dimension: one value shared by all dimensions is repeated"""
    return v.expand(*v.shape[:-1], width).clone() if v.shape[-1] == 1 and width > 1 else v


def _kernel_choice(who: str, kernel, nu: float, ard: bool, d: int):
    """(family: a class of STATIONARY_KERNELS, nu, ard, start) of the ``kernel`` argument of ExactGP / DirichletExactGP;
    start: the kernel object whose values the raw parameters start from, or None"""
    start = None
    if isinstance(kernel, type) and kernel in STATIONARY_KERNELS:
        family = kernel
    elif isinstance(kernel, BaseKernel):
        if not isinstance(kernel, STATIONARY_KERNELS):
            raise TypeError(f"{who}: the kernel must be an ARDKernel, a MaternKernel, an RQKernel, a PeriodicKernel, a "
                            "LocallyPeriodicKernel or a TrendSeasonalKernel (a lengthscale and an outputscale to learn)")
        start, family = kernel, _FAMILIES[kernel.family]
        nu = getattr(kernel, "nu", nu)
        ard = kernel.lengthscale.numel() > 1 or d == 1 and ard
        for attr, per_dim in family.shape_blocks:  # per-dimension shape values need per-dimension raw values too
            ard = ard or per_dim and getattr(kernel, attr).numel() > 1
    else:
        if kernel not in _KERNEL_NAMES:
            raise ValueError(f"{who}: kernel must be one of {sorted(_KERNEL_NAMES)}, a kernel class or a kernel object, got {kernel!r}")
        name, named_nu = _KERNEL_NAMES[kernel]
        family, nu = _FAMILIES[name], named_nu if named_nu is not None else nu
    if family is MaternKernel and float(nu) not in MaternKernel.KINDS:
        raise ValueError(f"{who}: nu must be 0.5, 1.5 or 2.5, got {nu}")
    return family, (float(nu) if family is MaternKernel else None), bool(ard), start


class _ExactGPClasses:
    """What ExactGP and DirichletExactGP share: C independent exact GPs on the shared x, class c with a constant mean m_c,
    K_c = s_c kappa(x, x; l_c) and K_y,c = K_c + diag(v_c) + sigma_c I, parametrised as gpytorch does: ``lengthscale =
    softplus(raw)``, ``outputscale = softplus(raw)``, ``noise = 1e-4 + softplus(raw)``, the mean constant itself; every raw
    value starts at 0.  ``raw`` is seen as (C, 3 + nls + shape columns) rows: mean, raw noise, raw outputscale, the nls raw
    lengthscales (d of them, or one shared by all dimensions), then the family's raw shape values, ``softplus(raw)`` each:
    none for RBF and Matern, raw alpha for the rational-quadratic kernel, the nls raw period lengths for the periodic kernel,
    the nls raw periodic lengthscales and then the nls raw period lengths for the locally periodic kernel, the nls raw
    seasonal lengthscales, periodic lengthscales and period lengths and then the raw seasonal outputscale for the
    trend-plus-seasonal kernel (a family's shape blocks in their declared order, kernel._StationaryKernel.shape_blocks)
    -- _lib.kernel_shape_params with the nls raw lengthscales in the place of the library's d.  x (n, d), the targets (C, n)
    and the fixed noise v (C, n), or None, are kept as given and uploaded once, on the first evaluation on the device.  One
    evaluation of all classes is ONE library call with one read-back, ``pls_gp_mll_grad_classes``: 4 + d + shape
    parameters outputs per class."""

    def __init__(self, who: str, x: torch.Tensor, targets: torch.Tensor, fixed_noise: torch.Tensor | None, kernel, nu: float,
                 ard: bool):
        x = x.detach()
        self.x = (x if x.dim() == 2 else x[:, None]).to(torch.float64)
        self.n, self.d = self.x.shape
        self._targets, self.fixed_noise = targets, fixed_noise
        self._family, self.nu, self.ard, start = _kernel_choice(who, kernel, nu, ard, self.d)
        self.kernel_name = self._family.family
        self.kind = self._family.kind if self.nu is None else MaternKernel.KINDS[self.nu]
        self._nls = nls = self.d if self.ard else 1
        raw = torch.zeros(targets.shape[0], 3 + nls + L.kernel_shape_params(self.kind, nls), dtype=torch.float64)
        if start is not None:
            raw[:, 2] = _inverse_softplus(torch.tensor(start.outputscale, dtype=torch.float64))
            for name, columns, _ in self._raw_blocks():
                v = torch.as_tensor(getattr(start, name), dtype=torch.float64).reshape(-1)
                assert v.numel() in (1, raw[:, columns].shape[1]), f"the kernel's {name.replace('_', ' ')}s do not fit the data"
                raw[:, columns] = _inverse_softplus(_repeated(v, raw[:, columns].shape[1]))
        self.raw = torch.nn.Parameter(raw)
        self._dev: dict = {}

    def _raw_blocks(self) -> list:
        """[(attribute, its columns of ``raw``, per_dim)]: the lengthscale block, then the family's shape blocks in their
        declared order; a per-dimension block has nls columns and the library reads d values of it, any other has one"""
        blocks, at = [], 3
        for name, per_dim in (("lengthscale", True),) + tuple(self._family.shape_blocks):
            width = self._nls if per_dim else 1
            blocks.append((name, slice(at, at + width), per_dim))
            at += width
        return blocks

    # ---- parameters -------------------------------------------------------------------------------------------------
    def raw_parameters(self) -> torch.Tensor:
        """A copy of ``raw`` (float64, CPU; the order is in the class docstring)."""
        return self.raw.detach().clone()

    def set_raw_parameters(self, raw: torch.Tensor):
        raw = torch.as_tensor(raw, dtype=torch.float64)
        assert raw.shape == self.raw.shape, f"raw parameters of shape {tuple(self.raw.shape)} expected, got {tuple(raw.shape)}"
        with torch.no_grad():
            self.raw.copy_(raw)
        return self

    def _natural(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(mean constant (C), noise (C), outputscale (C), lengthscale (C, d): a shared one repeated)"""
        raw = self.raw.detach().reshape(self._targets.shape[0], -1)
        ls = _repeated(_softplus(raw[:, 3:3 + self._nls]), self.d)
        return raw[:, 0].clone(), NOISE_LOWER_BOUND + _softplus(raw[:, 1]), _softplus(raw[:, 2]), ls

    def _shape(self, attr: str | None = None) -> torch.Tensor:
        """(C, shape parameters) the family's shape values as the library reads and differentiates them, block after block:
        softplus(raw) with a value shared by all dimensions repeated within its block; (C, 0) for a family without.
        ``attr``: the public property that asks, and gets its block alone; AttributeError when the family has no block of
        that name"""
        if attr is not None and attr not in dict(self._family.shape_blocks):
            raise AttributeError(f"the {self.kernel_name} kernel has no {attr}")
        raw = self.raw.detach().reshape(self._targets.shape[0], -1)
        blocks = [_repeated(_softplus(raw[:, columns]), self.d if per_dim else 1)
                  for name, columns, per_dim in self._raw_blocks()[1:] if attr in (None, name)]
        return torch.cat(blocks, dim=1) if blocks else raw[:, :0].clone()

    @property
    def alpha(self) -> torch.Tensor:
        """(C) the shape of the rational-quadratic kernel; AttributeError for the other kernels"""
        return self._shape("alpha")[:, 0]

    @property
    def period_length(self) -> torch.Tensor:
        """(C, d) the period lengths of the periodic, the locally periodic and the trend-plus-seasonal kernel (a shared one
        repeated); AttributeError for the other kernels"""
        return self._shape("period_length")

    @property
    def periodic_lengthscale(self) -> torch.Tensor:
        """(C, d) the lengthscales of the periodic factor of the locally periodic and the trend-plus-seasonal kernel (a shared
        one repeated); AttributeError for the other kernels"""
        return self._shape("periodic_lengthscale")

    @property
    def seasonal_lengthscale(self) -> torch.Tensor:
        """(C, d) the envelope lengthscales of the trend-plus-seasonal kernel's seasonal term (a shared one repeated);
        AttributeError for the other kernels"""
        return self._shape("seasonal_lengthscale")

    @property
    def seasonal_outputscale(self) -> torch.Tensor:
        """(C) the outputscale of the trend-plus-seasonal kernel's seasonal term; AttributeError for the other kernels"""
        return self._shape("seasonal_outputscale")[:, 0]

    def _library_lengthscale(self) -> torch.Tensor:
        """(C, d + shape parameters): the lengthscales, then the shape values, as the library reads them"""
        return torch.cat([self._natural()[3], self._shape()], dim=1)

    @property
    def mean_constant(self) -> torch.Tensor:
        return self._natural()[0]

    @property
    def noise(self) -> torch.Tensor:
        """(C) the learned noise sigma_c"""
        return self._natural()[1]

    @property
    def outputscale(self) -> torch.Tensor:
        return self._natural()[2]

    @property
    def lengthscale(self) -> torch.Tensor:
        """(C, d) lengthscales (a shared one repeated)."""
        return self._natural()[3]

    def _make_kernel(self, lengthscale: torch.Tensor, outputscale: float, shape: torch.Tensor) -> BaseKernel:
        """``shape``: the family's shape values (a row of ``_shape()``; empty for a family without)"""
        keywords, at = {} if self.nu is None else {"nu": self.nu}, 0
        for name, per_dim in self._family.shape_blocks:
            width = self.d if per_dim else 1
            keywords[name] = shape[at:at + width]
            at += width
        return self._family(lengthscale, outputscale, **keywords)

    def _class_kernel(self, c: int) -> BaseKernel:
        """the kernel of class c at the current parameters"""
        _, _, s, ls = self._natural()
        return self._make_kernel(ls[c], float(s[c]), self._shape()[c])

    # ---- the loss ---------------------------------------------------------------------------------------------------
    def chain_rule(self, out: torch.Tensor) -> Tuple[float, torch.Tensor]:
        """(-sum_c mll_c / n, its gradient with respect to ``raw``, in the shape of ``raw``) from the (C, 4 + d + shape
        parameters) outputs of pls_gp_mll_grad_classes (per class: value, d/d mean, d/d noise, d/d log outputscale,
        d/d log lengthscale_k, then d/d log of every shape value) at the current parameters: host arithmetic only.  The
        derivatives of a raw value that the library reads repeated, once per dimension (``ard=False``: the shared
        lengthscale, the shared period length), are summed, block by block."""
        raw = self.raw.detach().reshape(self._targets.shape[0], -1)
        out = torch.as_tensor(out, dtype=torch.float64)
        assert out.numel() == raw.shape[0] * self._outputs
        out = out.reshape(raw.shape[0], self._outputs)
        slope = torch.sigmoid(raw)  # d softplus(raw) / d raw
        g = torch.empty_like(raw)
        g[:, 0] = out[:, 1]
        g[:, 1] = out[:, 2] * slope[:, 1]
        g[:, 2] = out[:, 3] / _softplus(raw[:, 2]) * slope[:, 2]
        natural, at = self._library_lengthscale(), 0
        for _, columns, per_dim in self._raw_blocks():
            width = self.d if per_dim else 1
            d_natural = out[:, 4 + at:4 + at + width] / natural[:, at:at + width]
            shared = width != g[:, columns].shape[1]
            g[:, columns] = (d_natural.sum(dim=1, keepdim=True) if shared else d_natural) * slope[:, columns]
            at += width
        return -float(out[:, 0].sum()) / self.n, (-g / self.n).reshape(self.raw.shape)

    @property
    def _outputs(self) -> int:
        """outputs of one class of pls_gp_mll_grad_classes"""
        return 4 + self.d + L.kernel_shape_params(self.kind, self.d)

    def _device_state(self) -> dict:
        if not self._dev:
            x = _dev(self.x)
            c, width = self._targets.shape[0], self._outputs
            nbytes = int(L.load().pls_gp_mll_classes_workspace_bytes_kind(self.kind, self.n, self.d, c))
            self._dev = {
                "x": x, "y": _dev(self._targets.contiguous()),
                "fixed": _dev(self.fixed_noise.contiguous()) if self.fixed_noise is not None else None,
                "ws": torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device),
                # the C rows of outputs and behind them the C int32 info words: one read-back per evaluation
                "out": torch.zeros(c * width + (c + 1) // 2, dtype=torch.float64, device=x.device),
            }
        return self._dev

    def _evaluate(self, jitter: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """One pls_gp_mll_grad_classes call at the current parameters: (the (C, 4 + d + shape parameters) outputs on the
        CPU, info (C))."""
        st = self._device_state()
        c, width = self._targets.shape[0], self._outputs
        mean, noise, s, _ = self._natural()
        ls = st["x"].new_tensor(self._library_lengthscale().tolist()).contiguous()
        host = (ctypes.c_double * c)
        s, noise, mean = host(*s.tolist()), host(*noise.tolist()), host(*mean.tolist())
        out, ws, fixed = st["out"], st["ws"], st["fixed"]
        L.check(
            L.load().pls_gp_mll_grad_classes(self.kind, st["x"].data_ptr(), self.n, self.d, c, ls.data_ptr(),
                                             ctypes.cast(s, ctypes.c_void_p), ctypes.cast(noise, ctypes.c_void_p),
                                             ctypes.cast(mean, ctypes.c_void_p), fixed.data_ptr() if fixed is not None else None,
                                             self.n, st["y"].data_ptr(), self.n, float(jitter), out.data_ptr(),
                                             out.data_ptr() + 8 * c * width, ws.data_ptr(), ws.numel() * 8, L.stream_ptr()),
            "pls_gp_mll_grad_classes",
        )
        got = out.cpu()
        return got[: c * width].reshape(c, width), got[c * width:].view(torch.int32)[:c].clone()

    def loss_and_grad(self) -> Tuple[float, torch.Tensor]:
        """(-sum_c mll_c / n, its gradient with respect to ``raw``): gpytorch's ``-mll(model(x), y)``, summed over the
        classes, and ``backward()``.  When ANY class meets a non-positive pivot the whole call is retried with
        psd_safe_cholesky's jitters (1e-8, 1e-7, 1e-6), a warning per attempt, NotPSDError after the last."""
        attempts = [0.0] + [CHOLESKY_JITTER * 10**i for i in range(CHOLESKY_MAX_TRIES)]
        for jit in attempts:
            if jit > 0.0:
                warnings.warn(f"A not p.d., added jitter of {jit:.1e} to the diagonal", RuntimeWarning, stacklevel=2)
            out, info = self._evaluate(jit)
            if not info.any():
                return self.chain_rule(out)
        raise NotPSDError(f"Matrix not positive definite after repeatedly adding jitter up to {attempts[-1]:.1e}.")

    # ---- prediction -------------------------------------------------------------------------------------------------
    def _predict_class(self, c: int, x_test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(latent mean, latent variance) of class c at x_test (t, d), float64 on the device: m_c + k*^T alpha_c and
        k** - |Lc^-1 k*|^2 with K_y,c = Lc Lc^T, alpha_c = K_y,c^-1 (y_c - m_c) and k** the kernel's prior variance."""
        st = self._device_state()
        mean_c, noise, _, _ = (v[c] for v in self._natural())
        mean_c, noise = float(mean_c), float(noise)
        kern = self._class_kernel(c)
        ky = kern(st["x"], st["x"])
        ky.diagonal().add_(st["fixed"][c] + noise if st["fixed"] is not None else noise)
        factor = cholesky_factor(ky)
        alpha = factor.solve((st["y"][c] - mean_c)[:, None].contiguous())
        ks = kern(st["x"], x_test if x_test.dim() == 2 else x_test[:, None])  # (n, t): k-major
        t = ks.shape[1]
        mean = torch.empty((t, 1), dtype=torch.float64, device=ks.device)
        L.check(L.load().pls_gemm_tn(ks.data_ptr(), L.ld(ks), alpha.data_ptr(), 1, mean.data_ptr(), 1, t, 1, self.n, 1.0, 0.0,
                                     L.stream_ptr()), "pls_gemm_tn")
        v = factor.forward_solve(ks)
        return mean[:, 0] + mean_c, kern.prior_variance - v.square().sum(dim=0)


class ExactGP(_ExactGPClasses):
    """Exact GP regression with a constant mean, a scaled stationary kernel and Gaussian noise: the one-class case of
    _ExactGPClasses, without fixed noise.

    ``raw`` is ONE float64 CPU tensor, in this order::

        raw[0]   the mean constant
        raw[1]   raw noise
        raw[2]   raw outputscale
        raw[3:3 + nls]  raw lengthscales: nls = d of them (``ard=True``) or one shared by all dimensions (``ard=False``)
        raw[3 + nls:]   the family's raw shape values: raw alpha (rational quadratic), the nls raw period lengths (periodic),
                        the nls raw periodic lengthscales and then the nls raw period lengths (locally periodic), the nls raw
                        seasonal lengthscales, periodic lengthscales, period lengths and then the raw seasonal outputscale
                        (trend plus seasonal)

    ``kernel``: "rbf", "rq" or "matern" (with ``nu``); "matern12" / "matern32" / "matern52" name nu as well; one of the classes
    kernel.STATIONARY_KERNELS names its family likewise (the periodic, the locally periodic and the trend-plus-seasonal family
    have no name here: ``kernel=PeriodicKernel``, ``kernel=LocallyPeriodicKernel``, ``kernel=TrendSeasonalKernel``;
    ``train_exact_gp`` and ``exact_gp_runner`` take "periodic", "locally_periodic" and "trend_seasonal"); an instance of them gives the kind and the starting values (as the reference's ``deepcopy(kernel)``).
    x (n, d) and y (n) are kept as given."""

    def __init__(self, x: torch.Tensor, y: torch.Tensor, kernel="rbf", nu: float = 2.5, ard: bool = True):
        self.y = y.detach().reshape(-1).to(torch.float64)
        assert x.shape[0] == self.y.shape[0] and x.shape[0] > 0, "x (n, d) and y (n) must share n > 0"
        super().__init__("ExactGP", x, self.y[None, :], None, kernel, nu, ard)
        self.raw = torch.nn.Parameter(self.raw.detach()[0].clone())

    def set_raw_parameters(self, raw: torch.Tensor) -> "ExactGP":
        raw = torch.as_tensor(raw, dtype=torch.float64).reshape(-1)
        assert raw.numel() == self.raw.numel(), f"{self.raw.numel()} raw parameters expected, got {raw.numel()}"
        return super().set_raw_parameters(raw)

    @property
    def mean_constant(self) -> float:
        return float(self._natural()[0][0])

    @property
    def noise(self) -> float:
        return float(self._natural()[1][0])

    @property
    def outputscale(self) -> float:
        return float(self._natural()[2][0])

    @property
    def lengthscale(self) -> torch.Tensor:
        """d lengthscales (a shared one repeated)."""
        return self._natural()[3][0]

    @property
    def alpha(self) -> float:
        """the shape of the rational-quadratic kernel; AttributeError for the other kernels"""
        return float(self._shape("alpha")[0, 0])

    @property
    def period_length(self) -> torch.Tensor:
        """the d period lengths of the periodic and the locally periodic kernel (a shared one repeated); AttributeError for
        the other kernels"""
        return self._shape("period_length")[0]

    @property
    def periodic_lengthscale(self) -> torch.Tensor:
        """the d lengthscales of the periodic factor of the locally periodic and the trend-plus-seasonal kernel (a shared one
        repeated); AttributeError for the other kernels"""
        return self._shape("periodic_lengthscale")[0]

    @property
    def seasonal_lengthscale(self) -> torch.Tensor:
        """the d envelope lengthscales of the trend-plus-seasonal kernel's seasonal term (a shared one repeated); AttributeError
        for the other kernels"""
        return self._shape("seasonal_lengthscale")[0]

    @property
    def seasonal_outputscale(self) -> float:
        """the outputscale of the trend-plus-seasonal kernel's seasonal term; AttributeError for the other kernels"""
        return float(self._shape("seasonal_outputscale")[0, 0])

    @property
    def kernel(self) -> BaseKernel:
        """The fitted base kernel: goes straight into PLSKernel and the inducing-point selectors."""
        return self._class_kernel(0)

    def evaluate_on_device(self, jitter: float = 0.0) -> Tuple[torch.Tensor, int]:
        """One pls_gp_mll_grad_classes call (one class) at the current parameters: (the 4 + d + shape parameters outputs on
        the CPU, info)."""
        out, info = self._evaluate(jitter)
        return out[0], int(info[0])

    def predict(self, x_test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(mean, latent variance, observation variance) at x_test (t, d), float64 on the device:
        c + k*^T alpha,  k** - |Lc^-1 k*|^2  and that plus the noise, with K_y = Lc Lc^T and alpha = K_y^-1 (y - c)."""
        mean, var = self._predict_class(0, x_test)
        return mean, var, var + self.noise

    def predict_mean(self, x_test: torch.Tensor) -> torch.Tensor:
        """The mean of ``predict`` alone, (t,) float64 on the device: c + sum_j k(x*_i, x_j) alpha_j in ONE
        ``pls_kernel_mean`` call -- no n x t matrix is built and no variance solve runs (the reference's
        ``model(experiment_data.train.x)`` at experiments/uci/regression/main.py:231 computes both and
        ``estimate_student_parameters`` keeps the mean).  alpha = K_y^-1 (y - c) is kept for the next call: the cache key
        is a clone of the raw parameter values, compared with ``torch.equal``, so ``set_raw_parameters`` or an optimiser
        step invalidates it."""
        st = self._device_state()
        cached = st.get("alpha")
        if cached is None or not torch.equal(cached[0], self.raw.detach()):
            mean_c, noise, s, _ = (v[0] for v in self._natural())
            ky = self._class_kernel(0)(st["x"], st["x"])
            ky.diagonal().add_(float(noise))
            alpha = cholesky_factor(ky).solve((st["y"][0] - float(mean_c))[:, None].contiguous())
            ls = self._library_lengthscale()[0]
            cached = (self.raw.detach().clone(), alpha.reshape(-1).contiguous(), st["x"].new_tensor(ls.tolist()).contiguous(),
                      float(s), float(mean_c))
            st["alpha"] = cached
        _, alpha, ls, s, mean_c = cached
        xt = _dev(x_test.detach() if x_test.dim() == 2 else x_test.detach()[:, None]).contiguous()
        assert xt.shape[1] == self.d, f"x_test has {xt.shape[1]} columns, the model {self.d}"
        out = torch.empty(xt.shape[0], dtype=torch.float64, device=xt.device)
        L.check(L.load().pls_kernel_mean(self.kind, st["x"].data_ptr(), self.n, self.d, ls.data_ptr(), s, mean_c,
                                         alpha.data_ptr(), xt.data_ptr(), xt.shape[0], out.data_ptr(), L.stream_ptr()),
                "pls_kernel_mean")
        return out


# ---- sparse variational GP (fixed kernel, fixed inducing points, Gaussian likelihood) ------------------------------------
#: gpytorch's jitter on k(Z, Z) for float64 data (settings.variational_cholesky_jitter; 1e-4 for float32 data)
SVGP_JITTER = 1e-6
SVGP_M_MAX = 256


def _kernel_diagonal(kernel, x: torch.Tensor) -> torch.Tensor:
    """k(x_i, x_i) for every row of the device matrix x, without the n x n Gram matrix."""
    from .kernel import LinearKernel, PLSKernel, _StationaryKernel

    if isinstance(kernel, _StationaryKernel):
        return torch.full((x.shape[0],), float(kernel.prior_variance), dtype=torch.float64, device=x.device)
    if isinstance(kernel, LinearKernel):
        return x.square().sum(dim=1)
    if isinstance(kernel, PLSKernel):
        s = kernel.approximation_samples.detach().cpu().to(torch.float64)
        s = (s if s.dim() == 2 else s[:, None]).unique(dim=0)
        return kernel.base_kernel(s, x).square().sum(dim=0) / s.shape[0]
    return torch.cat([kernel(c, c).diagonal() for c in x.split(1024)])


class SVGP:
    """The reference's SVGP baseline (src/gaussian_process/svgp.py:6-49) as every driver trains it (``is_fixed=True``): the
    kernel and the inducing points are frozen; the variational mean ``m``, the variational Cholesky factor ``L_s``, the
    constant mean ``c`` and the raw likelihood noise ``rho`` (noise = softplus(rho) + 1e-4) live on the device and are
    learned by plain SGD on the minibatch ELBO.  The arithmetic is gpytorch 1.15's whitened VariationalStrategy +
    CholeskyVariationalDistribution + VariationalELBO + GaussianLikelihood AS RECALLED (include/plship.h states the
    formulas; they are the contract).  Everything that depends on the kernel is computed once, in ``fit_data``; one
    evaluation is ``pls_svgp_elbo_grad``, one epoch ``pls_svgp_sgd_epoch``, a prediction ``pls_svgp_predict``.

    ``likelihood``: ``"gaussian"`` or a likelihood object (likelihoods.py).  A ``BernoulliLikelihood`` (labels in {0, 1}, no
    noise) or a ``StudentTLikelihood`` (fixed degrees of freedom, noise = softplus(rho) WITHOUT the 1e-4 floor) takes the
    20-node Gauss-Hermite epilogue through ``pls_svgp_lik_elbo_grad`` / ``_sgd_epoch`` / ``_predict``; a
    ``GaussianLikelihood`` is the closed-form path of ``"gaussian"``.

    ``kernel``: any kernel callable of the package (PLSKernel, ARDKernel, MaternKernel, RQKernel, PeriodicKernel, LinearKernel).  ``noise``: the
    starting likelihood noise (the likelihood object's own, else raw value 0, when None).  ``m`` starts at ``mean_init_std`` times standard normals from
    torch's global generator (drawn here, on the host), ``L_s`` at the identity."""

    def __init__(self, kernel, x_induce: torch.Tensor, likelihood: "str | _Likelihood" = "gaussian", noise: float | None = None,
                 mean_constant: float = 0.0, learn_inducing_locations: bool = False, jitter: float = SVGP_JITTER,
                 mean_init_std: float = 1e-3):
        if learn_inducing_locations:
            raise NotImplementedError("SVGP: learn_inducing_locations=True is not supported: the inducing points and the "
                                      "kernel are fixed (the reference's is_fixed=True); only the variational mean, the "
                                      "variational Cholesky factor, the constant mean and the noise are learned")
        if not isinstance(likelihood, _Likelihood) and likelihood != "gaussian":
            raise NotImplementedError(f"SVGP: likelihood {likelihood!r} is not supported: only 'gaussian' is "
                                      "(Bernoulli and Student-t are likelihood OBJECTS: "
                                      "BernoulliLikelihood(), StudentTLikelihood(deg_free))")
        z = x_induce.detach()
        self.x_induce = (z if z.dim() == 2 else z[:, None]).to(torch.float64)
        self.m = self.x_induce.shape[0]
        if not 1 <= self.m <= SVGP_M_MAX:
            raise ValueError(f"SVGP: {self.m} inducing points are not supported: 1 to {SVGP_M_MAX} are")
        self.kernel, self.jitter, self.likelihood = kernel, float(jitter), likelihood
        self._lik = likelihood if isinstance(likelihood, _Likelihood) else GaussianLikelihood()
        floor = self._lik.noise_floor
        if noise is not None and floor is None:
            raise AttributeError(f"SVGP: a {type(self._lik).__name__} has no noise to set")
        if noise is None:
            noise = self._lik.noise
        rho = 0.0
        if noise is not None:
            if not float(noise) > floor:
                raise ValueError(f"SVGP: the noise must exceed {floor}")
            rho = float(_inverse_softplus(torch.tensor(float(noise) - floor, dtype=torch.float64)))
        mean = torch.zeros(self.m, dtype=torch.float64)
        if mean_init_std:
            mean = float(mean_init_std) * torch.randn(self.m, dtype=torch.float64)
        self._start = (mean, float(mean_constant), rho)
        self._dev: dict = {}
        self.n = 0

    # ---- setup ------------------------------------------------------------------------------------------------------
    def _state(self) -> dict:
        if not self._dev:
            from .basis.base import alloc_matrix
            mean, c, rho = self._start
            z = _dev(self.x_induce)
            kzz = self.kernel(z, z)
            kzz.diagonal().add_(self.jitter)
            ls = alloc_matrix(self.m, self.m, z.device)
            ls.copy_(torch.eye(self.m, dtype=torch.float64))
            self._dev = {"z": z, "factor": cholesky_factor(kzz), "mean": _dev(mean), "Ls": ls,
                         "scalars": torch.tensor([c, rho], dtype=torch.float64, device=z.device),
                         "out": torch.zeros(5, dtype=torch.float64, device=z.device), "ws": None}
        return self._dev

    def _whitened_rows(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(At, q) of the points x: the rows of (L^-1 k(Z, x))^T with an even leading dimension, and
        k(x_i, x_i) + jitter - |row i|^2"""
        st = self._state()
        a = st["factor"].forward_solve(self.kernel(st["z"], x))  # (M, t)
        t = a.shape[1]
        at = torch.zeros((t, (self.m + 1) & ~1), dtype=torch.float64, device=a.device)[:, : self.m]
        at.copy_(a.T)
        q = _kernel_diagonal(self.kernel, x) + self.jitter - a.square().sum(dim=0)
        return at, q.contiguous()

    def fit_data(self, x: torch.Tensor, y: torch.Tensor) -> "SVGP":
        """The once-per-model setup: K_zz + jitter I = L L^T (retried with growing jitter as psd_safe_cholesky does;
        NotPSDError after the last attempt), At = (L^-1 k(Z, X))^T and q on the device."""
        if self._lik.code == L.SVGP_BERNOULLI:
            labels = torch.as_tensor(y).detach().reshape(-1)
            if not bool(((labels == 0) | (labels == 1)).all()):
                raise ValueError("SVGP: a BernoulliLikelihood needs labels in {0, 1}")
        st = self._state()
        xd = _dev(x if x.dim() == 2 else x[:, None])
        yd = _dev(y.reshape(-1))
        assert xd.shape[0] == yd.shape[0] and xd.shape[0] > 0, "x (n, d) and y (n) must share n > 0"
        self.n = xd.shape[0]
        at, q = self._whitened_rows(xd)
        quadrature = self._lik.code != L.SVGP_GAUSSIAN
        lik_desc = L.SvgpLikDesc()
        lik_desc.deg_free = self._lik.deg_free
        desc = lik_desc.base if quadrature else L.SvgpDesc()
        desc.At, desc.ldat, desc.q, desc.y = at.data_ptr(), at.stride(0), q.data_ptr(), yd.data_ptr()
        desc.n, desc.m, desc.likelihood = self.n, self.m, self._lik.code
        st.update(At=at, q=q, y=yd, desc=lik_desc if quadrature else desc, ws=None)
        return self

    def _entry(self, name: str):
        """(the library entry ``pls_svgp[_lik]_<name>`` of this model's likelihood, its name)"""
        full = f"pls_svgp_lik_{name}" if self._lik.code != L.SVGP_GAUSSIAN else f"pls_svgp_{name}"
        return getattr(L.load(), full), full

    def _workspace(self, batch: int) -> torch.Tensor:
        st = self._state()
        nbytes = int(L.load().pls_svgp_workspace_bytes(self.n, self.m, batch))
        if st["ws"] is None or st["ws"].numel() * 8 < nbytes:
            st["ws"] = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=st["z"].device)
        return st["ws"]

    def _fitted(self) -> dict:
        st = self._state()
        if "desc" not in st:
            raise RuntimeError("SVGP: call fit_data(x, y) first")
        return st

    # ---- parameters -------------------------------------------------------------------------------------------------
    @property
    def variational_mean(self) -> torch.Tensor:
        """m (M), the device tensor itself"""
        return self._state()["mean"]

    @property
    def chol_variational_covar(self) -> torch.Tensor:
        """L_s (M, M) on the device; only its lower triangle and diagonal mean anything"""
        return self._state()["Ls"]

    @property
    def scalars(self) -> torch.Tensor:
        """the device pair (c, rho)"""
        return self._state()["scalars"]

    @property
    def mean_constant(self) -> float:
        return float(self._state()["scalars"][0])

    @property
    def noise(self) -> float:
        """the likelihood's noise: softplus(rho) + 1e-4 (Gaussian), softplus(rho) (Student-t); Bernoulli has none"""
        floor = self._lik.noise_floor
        if floor is None:
            raise AttributeError(f"SVGP: a {type(self._lik).__name__} has no noise")
        rho = self._state()["scalars"][1].cpu()
        return floor + float(torch.clamp(rho, min=0.0) + torch.log1p(torch.exp(-rho.abs())))

    # ---- the ELBO ---------------------------------------------------------------------------------------------------
    def evaluate_on_device(self, idx: torch.Tensor | None = None, gradients: bool = True
                           ) -> Tuple[torch.Tensor, torch.Tensor | None, torch.Tensor | None]:
        """One pls_svgp_elbo_grad call: (out (5, device): ELBO, d/dc, d/drho, (1/B) sum l_i, KL; d/dm (M); d/dL_s (M, M),
        lower triangle, zeros above).  ``idx``: int64 indices of the minibatch, all rows in order when None."""
        st = self._fitted()
        if idx is not None:
            idx = idx.to(device=st["z"].device, dtype=torch.int64).contiguous()
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n):
                raise IndexError(f"SVGP: minibatch indices must lie in 0 .. {self.n - 1}")
        b = self.n if idx is None else idx.numel()
        ws = self._workspace(b)
        gm = gl = None
        if gradients:
            gm = torch.empty(self.m, dtype=torch.float64, device=ws.device)
            gl = torch.zeros((self.m, self.m), dtype=torch.float64, device=ws.device)
        fn, name = self._entry("elbo_grad")
        L.check(fn(ctypes.byref(st["desc"]), st["mean"].data_ptr(), st["Ls"].data_ptr(), L.ld(st["Ls"]), st["scalars"].data_ptr(),
                   L.ptr(idx), b, st["out"].data_ptr(), L.ptr(gm), L.ptr(gl), self.m, ws.data_ptr(), ws.numel() * 8,
                   L.stream_ptr()), name)
        return st["out"], gm, gl

    def elbo_and_grad(self, idx: torch.Tensor | None = None) -> Tuple[float, dict]:
        """(ELBO of the minibatch, its gradients): ``variational_mean`` (M) and ``chol_variational_covar`` (M, M, lower
        triangle) on the device, ``mean_constant`` and ``raw_noise`` as floats."""
        out, gm, gl = self.evaluate_on_device(idx)
        host = out.cpu()
        return float(host[0]), {"variational_mean": gm, "chol_variational_covar": gl, "mean_constant": float(host[1]),
                                "raw_noise": float(host[2])}

    def sgd_epoch(self, perm: torch.Tensor, batch_size: int, learning_rate: float, train_mean: bool = True,
                  train_noise: bool = True) -> torch.Tensor:
        """One pls_svgp_sgd_epoch call over the device index list ``perm`` (n int64): every minibatch step on the device,
        then the full-data loss of the updated state, returned as a 1-element device tensor."""
        st = self._fitted()
        perm = perm.to(device=st["z"].device, dtype=torch.int64).contiguous()
        assert perm.numel() == self.n, "perm must list all n rows"
        ws = self._workspace(min(int(batch_size), self.n))
        loss = torch.empty(1, dtype=torch.float64, device=ws.device)
        flags = (L.SVGP_TRAIN_MEAN if train_mean else 0) | (L.SVGP_TRAIN_NOISE if train_noise else 0)
        fn, name = self._entry("sgd_epoch")
        L.check(fn(ctypes.byref(st["desc"]), st["mean"].data_ptr(), st["Ls"].data_ptr(), L.ld(st["Ls"]), st["scalars"].data_ptr(),
                   perm.data_ptr(), int(batch_size), float(learning_rate), flags, loss.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                   L.stream_ptr()), name)
        return loss

    # ---- prediction -------------------------------------------------------------------------------------------------
    def predict(self, x_test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(mean, latent variance, observation variance) at x_test (t, d), float64 on the device: c + a* . m,
        q* + |L_s^T a*|^2 and that plus the noise; with a Student-t likelihood the third is v + noise nu / (nu - 2), with a
        Bernoulli likelihood p (1 - p) at p = Phi(mean / sqrt(1 + v)) (pls_svgp_lik_predict's obs_out)."""
        st = self._state()
        xt = _dev(x_test if x_test.dim() == 2 else x_test[:, None])
        at, q = self._whitened_rows(xt)
        t = xt.shape[0]
        mean = torch.empty(t, dtype=torch.float64, device=xt.device)
        var = torch.empty(t, dtype=torch.float64, device=xt.device)
        if self._lik.code != L.SVGP_GAUSSIAN:
            obs = torch.empty(t, dtype=torch.float64, device=xt.device)
            desc = L.SvgpLikDesc()
            desc.base.likelihood, desc.deg_free = self._lik.code, self._lik.deg_free
            L.check(L.load().pls_svgp_lik_predict(ctypes.byref(desc), st["mean"].data_ptr(), st["Ls"].data_ptr(), L.ld(st["Ls"]),
                                                  st["scalars"].data_ptr(), at.data_ptr(), at.stride(0), q.data_ptr(), t, self.m,
                                                  mean.data_ptr(), var.data_ptr(), obs.data_ptr(), L.stream_ptr()),
                    "pls_svgp_lik_predict")
            return mean, var, obs
        L.check(L.load().pls_svgp_predict(st["mean"].data_ptr(), st["Ls"].data_ptr(), L.ld(st["Ls"]), st["scalars"].data_ptr(),
                                          at.data_ptr(), at.stride(0), q.data_ptr(), t, self.m, mean.data_ptr(), var.data_ptr(),
                                          L.stream_ptr()), "pls_svgp_predict")
        return mean, var, var + self.noise

    def predict_proba(self, x_test: torch.Tensor) -> torch.Tensor:
        """p(y = 1) at x_test under a BernoulliLikelihood: Phi(mean / sqrt(1 + latent variance)), float64 on the device"""
        if self._lik.code != L.SVGP_BERNOULLI:
            raise AttributeError("SVGP: predict_proba exists for a BernoulliLikelihood only")
        mean, var, _ = self.predict(x_test)
        return torch.special.ndtr(mean / torch.sqrt(1.0 + var))


# ---- the Student-t noise of the regression drivers --------------------------------------------------------------------
def student_t_sums_on_device(residuals: torch.Tensor, nu: float, s: float) -> Tuple[float, float, float]:
    """(A, B, C) = (sum log1p(u), sum u / (1 + u), sum u / (1 + u)^2), u_i = r_i^2 / (nu s^2), of device residuals from
    entries the library already has, with the Student-t ``pls_cost_desc`` at (nu, s) on the single column F = r, y = 0:
    the cost value is (nu + 1)/2 A (``pls_cost_value``), its derivative G_i = (nu + 1) r_i / (nu s^2 + r_i^2)
    (``pls_cost_derivative``) gives r^T G = (nu + 1) B and G^T G = (nu + 1)^2 C / (nu s^2) (one ``pls_gemm_tn``).  One
    read-back of three numbers."""
    r = L.require_gpu_tensor(residuals, "residuals").reshape(-1).contiguous()
    n = r.numel()
    lib = L.load()
    desc = L.CostDesc()
    desc.cost, desc.link, desc.deriv_mode = L.COST_STUDENT_T, L.LINK_IDENTITY, L.DERIV_REFERENCE
    desc.p[0], desc.p[1], desc.jitter = float(nu), float(s), 1e-10
    zero = torch.zeros(n, dtype=torch.float64, device=r.device)
    g = torch.empty((n, 1), dtype=torch.float64, device=r.device)
    out = torch.empty(4, dtype=torch.float64, device=r.device)
    ws_bytes = lib.pls_cost_value_workspace_bytes(n, 1)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=r.device)
    L.check(lib.pls_cost_value(desc, r.data_ptr(), 1, zero.data_ptr(), n, 1, out.data_ptr(), ws.data_ptr(), ws_bytes,
                               L.stream_ptr()), "pls_cost_value")
    L.check(lib.pls_cost_derivative(desc, r.data_ptr(), 1, zero.data_ptr(), n, 1, g.data_ptr(), 1, L.stream_ptr()),
            "pls_cost_derivative")
    _ops.gemm_tn(g, torch.stack([r, g[:, 0]], dim=1), out=out[2:4].view(1, 2))  # G^T [r G]: one contraction
    c, _, rtg, gtg = out.cpu().tolist()
    return 2.0 * c / (nu + 1.0), rtg / (nu + 1.0), nu * s * s * gtg / (nu + 1.0) ** 2


def _trigamma(x: float) -> float:
    """psi'(x) for x > 0: the recurrence psi'(x) = psi'(x + 1) + 1/x^2 up to x >= 15, then the asymptotic series through
    x^-15 (truncation below 1e-18 there); torch.special.polygamma(1, .) is good to 1e-10 only"""
    total = 0.0
    while x < 15.0:
        total += 1.0 / (x * x)
        x += 1.0
    w = 1.0 / (x * x)
    series = w * (1.0 / 6 + w * (-1.0 / 30 + w * (1.0 / 42 + w * (-1.0 / 30 + w * (5.0 / 66 + w * (-691.0 / 2730 + w * 7.0 / 6))))))
    return total + (1.0 / x + 0.5 * w + series / x)


def _student_t_pieces(n: int, nu: float, a: float, b: float, c: float, log_s: float):
    """(negative log-likelihood, its gradient and Hessian in (log nu, log s)) of n zero-location Student-t residuals from
    the three sums: with h(nu) = lgamma((nu + 1)/2) - lgamma(nu/2) - log(nu pi)/2,
    ll = n h - n log s - (nu + 1)/2 A;  d/dlog nu = n nu h' - nu A/2 + (nu + 1) B/2;  d/dlog s = -n + (nu + 1) B;
    d2/dlog nu2 = n nu (h' + nu h'') - nu A/2 + nu B - (nu + 1) C/2;  d2/dlog nu dlog s = nu B - (nu + 1) C;
    d2/dlog s2 = -2 (nu + 1) C."""
    half = torch.tensor([0.5 * (nu + 1.0), 0.5 * nu], dtype=torch.float64)
    psi, tri = torch.special.digamma(half).tolist(), (_trigamma(0.5 * (nu + 1.0)), _trigamma(0.5 * nu))
    h = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
    h1 = 0.5 * (psi[0] - psi[1]) - 0.5 / nu
    h2 = 0.25 * (tri[0] - tri[1]) + 0.5 / (nu * nu)
    nll = -(n * h - n * log_s - 0.5 * (nu + 1.0) * a)
    g = (-(n * nu * h1 - 0.5 * nu * a + 0.5 * (nu + 1.0) * b), -(-n + (nu + 1.0) * b))
    haa = -(n * nu * (h1 + nu * h2) - 0.5 * nu * a + nu * b - 0.5 * (nu + 1.0) * c)
    hab = -(nu * b - (nu + 1.0) * c)
    hbb = 2.0 * (nu + 1.0) * c
    return nll, g, (haa, hab, hbb)


def fit_student_t(residuals: torch.Tensor, deg_free_bounds: Tuple[float, float] = (1e-2, 1e6),
                  evaluate: Callable[[torch.Tensor, float, float], Tuple[float, float, float]] | None = None
                  ) -> Tuple[float, float]:
    """(deg_free, scale): the maximum-likelihood parameters of a zero-location Student-t for the residuals -- what
    ``scipy.stats.t.fit(residuals, floc=0)`` approximates with Nelder-Mead at experiments/uci/regression/main.py:124.

    Damped Newton in (log nu, log s) from nu = 1, s = rms(r): the Newton step (steepest descent of unit length where the
    Hessian of the negative log-likelihood is not positive definite; no step longer than 2 in either coordinate) is halved
    until the negative log-likelihood does not rise by more than its own rounding noise (1e-12 relative to |nll| + n);
    it stops when both steps are at or below 1e-12 or after 100 iterations.  The data enter through three sums per
    evaluation (``student_t_sums_on_device``: existing library entries, one read-back); ``evaluate(residuals, nu, s) ->
    (A, B, C)`` replaces that evaluation (a host helper drives the same loop without a device).  Where log nu reaches a bound
    (Gaussian residuals: the likelihood has no finite maximiser in nu) nu is clamped there, the one-dimensional Newton
    iteration in log s is finished and ONE warning is emitted.

    The maximiser may lie at or below nu = 2, where the Student-t variance does not exist and ``StudentTLikelihood``
    raises; the reference has the same limit (gpytorch's variance is infinite there)."""
    evaluate = evaluate if evaluate is not None else student_t_sums_on_device
    r = residuals.detach().reshape(-1).to(torch.float64)
    n = r.numel()
    rms = float(r.square().mean().sqrt())
    if not (n > 0 and math.isfinite(rms) and rms > 0.0):
        raise ValueError("fit_student_t: the residuals must be finite and not all zero")
    lo, hi = math.log(deg_free_bounds[0]), math.log(deg_free_bounds[1])
    if not lo <= 0.0 <= hi:
        raise ValueError("fit_student_t: deg_free_bounds must contain the starting value 1")

    def pieces(a_, b_):
        nu_, s_ = math.exp(a_), math.exp(b_)
        return _student_t_pieces(n, nu_, *evaluate(r, nu_, s_), b_)

    a, b, pinned = 0.0, math.log(rms), False
    nll, g, hess = pieces(a, b)
    for _ in range(100):
        haa, hab, hbb = hess
        if pinned:
            da, db = 0.0, -g[1] / hbb
        else:
            det = haa * hbb - hab * hab
            if haa > 0.0 and det > 0.0:
                da, db = -(hbb * g[0] - hab * g[1]) / det, -(haa * g[1] - hab * g[0]) / det
            else:
                norm = math.hypot(g[0], g[1])
                da, db = -g[0] / norm, -g[1] / norm
        shrink = max(1.0, abs(da) / 2.0, abs(db) / 2.0)
        da, db = da / shrink, db / shrink
        if not pinned and not lo < a + da < hi:
            pinned, a = True, (lo if a + da <= lo else hi)
            warnings.warn(f"fit_student_t: the degrees of freedom reached the bound {math.exp(a):.3g}; they are clamped "
                          "there and only the scale is fitted", RuntimeWarning, stacklevel=2)
            nll, g, hess = pieces(a, b)
            continue
        for _ in range(60):
            new = pieces(a + da, b + db)
            if new[0] <= nll + 1e-12 * (abs(nll) + n):
                break
            da, db = 0.5 * da, 0.5 * db
        a, b = a + da, b + db
        nll, g, hess = new
        if abs(da) <= 1e-12 and abs(db) <= 1e-12:
            break
    return math.exp(a), math.exp(b)


def estimate_student_parameters(y_actual: torch.Tensor, predictions: Sequence, deg_free_bounds: Tuple[float, float] = (1e-2, 1e6),
                                evaluate=None) -> Tuple[float, float]:
    """experiments/uci/regression/main.py:109-125: the residuals ``y_actual - mean_k`` are averaged over the models and a
    zero-location Student-t is fitted to them (``fit_student_t``; the reference calls ``scipy.stats.t.fit(.., floc=0)``).
    ``predictions``: one mean tensor per model (``ExactGP.predict_mean`` at all N training points); a tuple as ``predict``
    returns it stands for its first element.  The averaging runs where the means live (on the device).  The result
    feeds ``StudentTCost(deg_free, y, link, scale)``, ``StudentTLikelihood(deg_free)`` and the predictive noise of
    ``OrthonormalBasis``; it may lie at or below 2, where ``StudentTLikelihood`` raises (see ``fit_student_t``)."""
    means = [p[0] if isinstance(p, (tuple, list)) else p for p in predictions]
    if not means:
        raise ValueError("estimate_student_parameters: no predictions")
    y = torch.as_tensor(y_actual).detach().reshape(-1).to(device=means[0].device, dtype=torch.float64)
    residuals = torch.stack([y - m.detach().reshape(-1).to(torch.float64) for m in means], dim=1).mean(dim=1)
    return fit_student_t(residuals, deg_free_bounds, evaluate)


#: gpytorch's DirichletClassificationLikelihood: the Dirichlet concentration of a class that was not observed
ALPHA_EPSILON = 0.01


def dirichlet_targets(labels: torch.Tensor, number_of_classes: int | None = None, alpha_epsilon: float = ALPHA_EPSILON,
                      target_dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """(transformed targets, fixed noise), both (C, n) float64, of integer labels in 0 .. C - 1 (Milios et al. 2018 as
    gpytorch's DirichletClassificationLikelihood._prepare_targets states it): with a_ci = alpha_epsilon + [y_i == c],
    v_ci = log(1 / a_ci + 1) and y~_ci = log a_ci - v_ci / 2.  Both are rounded to ``target_dtype`` (gpytorch's ``dtype``
    argument, float32 by default) and then promoted to float64.  C defaults to ``labels.max() + 1``."""
    labels = torch.as_tensor(labels).detach().reshape(-1).cpu()
    if labels.numel() == 0:
        raise ValueError("dirichlet_targets: no labels")
    if labels.is_floating_point():
        if not torch.equal(labels, labels.round()):
            raise ValueError("dirichlet_targets: the labels must be integers")
    labels = labels.to(torch.int64)
    classes = int(labels.max()) + 1 if number_of_classes is None else int(number_of_classes)
    if classes < 1 or int(labels.min()) < 0 or int(labels.max()) >= classes:
        raise ValueError(f"dirichlet_targets: labels must lie in 0 .. {classes - 1}, got {int(labels.min())} .. {int(labels.max())}")
    if target_dtype not in (torch.float32, torch.float64):
        raise ValueError("dirichlet_targets: target_dtype must be torch.float32 or torch.float64")
    a = torch.full((classes, labels.numel()), float(alpha_epsilon), dtype=torch.float64)
    a[labels, torch.arange(labels.numel())] += 1.0
    v = torch.log(1.0 / a + 1.0)
    targets = torch.log(a) - 0.5 * v
    return targets.to(target_dtype).to(torch.float64), v.to(target_dtype).to(torch.float64)


class DirichletExactGP(_ExactGPClasses):
    """Exact-GP classification with the Dirichlet likelihood: ``number_of_classes`` independent GPs on the shared x, class c
    with a constant mean m_c, K_c = s_c kappa(x, x; l_c) and K_y,c = K_c + diag(v_c) + sigma_c I, where v_c is the fixed
    per-point noise of ``dirichlet_targets`` and sigma_c = 1e-4 + softplus(raw) the learned "second noise"
    (``learn_additional_noise=True``); regression targets are the transformed labels.  Replaces the batch-of-classes
    gpytorch model of experiments/curves/classification/main.py:162-192 and experiments/uci/classification/main.py:133-163.

    ``raw`` is ONE (C, 3 + nls + shape columns) float64 CPU parameter, row c in ExactGP's column order (mean, raw noise, raw
    outputscale, raw lengthscales, the family's raw shape values); every raw value starts at 0.  ``transformed_targets`` and ``fixed_noise`` are (C, n);
    ``fixed_noise=False`` leaves the fixed part out (``self.fixed_noise`` is then None): what the reference trains on
    when its subsample is smaller than its data.
    One evaluation of all classes is ONE library call with one read-back, ``pls_gp_mll_grad_classes``."""

    def __init__(self, x: torch.Tensor, labels: torch.Tensor, kernel="rbf", nu: float = 2.5, ard: bool = True,
                 number_of_classes: int | None = None, alpha_epsilon: float = ALPHA_EPSILON,
                 target_dtype: torch.dtype = torch.float32, fixed_noise: bool = True):
        self.labels = torch.as_tensor(labels).detach().reshape(-1).cpu().to(torch.int64)
        assert x.shape[0] == self.labels.shape[0] and x.shape[0] > 0, "x (n, d) and labels (n) must share n > 0"
        self.transformed_targets, v = dirichlet_targets(labels, number_of_classes, alpha_epsilon, target_dtype)
        self.number_of_classes = self.transformed_targets.shape[0]
        super().__init__("DirichletExactGP", x, self.transformed_targets, v if fixed_noise else None, kernel, nu, ard)

    @property
    def kernels(self) -> List[BaseKernel]:
        """The fitted kernel of every class."""
        return [self._class_kernel(c) for c in range(self.number_of_classes)]

    @property
    def kernel(self) -> BaseKernel:
        """ONE kernel for PLSKernel and the inducing-point selectors: the raw kernel parameters averaged over the classes,
        softplus applied afterwards (constructors.py:28-53 with one model)."""
        return construct_average_ard_kernel([self])

    def evaluate_on_device(self, jitter: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """One pls_gp_mll_grad_classes call at the current parameters: (the (C, 4 + d + shape parameters) outputs on the
        CPU, info (C))."""
        return self._evaluate(jitter)

    def predict(self, x_test: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(latent mean, latent variance), both (C, t) float64 on the device: per class m_c + k*^T alpha_c and
        k** - |Lc^-1 k*|^2 with K_y,c = Lc Lc^T and alpha_c = K_y,c^-1 (y~_c - m_c)."""
        rows = [self._predict_class(c, x_test) for c in range(self.number_of_classes)]
        return torch.stack([mean for mean, _ in rows]), torch.stack([var for _, var in rows])

    def predict_proba(self, x_test: torch.Tensor, number_of_samples: int = 256, seed: int = 0) -> torch.Tensor:
        """(t, C) class probabilities: the mean over ``number_of_samples`` draws of softmax(f), f_c ~ N(mean_c, var_c)
        independently (gpytorch's ``pred.sample(...).exp()`` normalised and averaged), on the library's Philox stream
        (pls_softmax_normal_mean): test point i draws under ``seed`` with step i."""
        mean, var = self.predict(x_test)
        return softmax_normal_mean(mean, var, number_of_samples, seed)


def softmax_normal_mean(mean: torch.Tensor, variance: torch.Tensor, number_of_samples: int = 256, seed: int = 0,
                        first_point: int = 0) -> torch.Tensor:
    """pls_softmax_normal_mean on (C, t) device tensors of latent means and variances -> (t, C) probabilities; column i
    draws under ``seed`` with step ``first_point + i``, so a long list of test points can be split into calls."""
    assert mean.dim() == 2 and mean.shape == variance.shape and mean.is_cuda and variance.is_cuda
    mean, variance = mean.to(torch.float64).contiguous(), variance.to(torch.float64).contiguous()
    c, t = mean.shape
    out = torch.empty((t, c), dtype=torch.float64, device=mean.device)
    L.check(L.load().pls_softmax_normal_mean(mean.data_ptr(), t, variance.data_ptr(), t, c, t, int(number_of_samples), int(seed),
                                             int(first_point), out.data_ptr(), c, L.stream_ptr()), "pls_softmax_normal_mean")
    return out


def train_exact_gp(x: torch.Tensor, y: torch.Tensor, kernel, seed: int, number_of_epochs: int, learning_rate: float,
                   early_stopper_patience: float, evaluate: Callable[[ExactGP], Tuple[float, torch.Tensor]] | None = None,
                   likelihood: str = "gaussian", number_of_classes: int | None = None, fixed_noise: bool = True,
                   ) -> Tuple[ExactGP, List[float]]:
    """experiments/trainers.py:15-52, statement for statement: seed, Adam over the raw parameters, and per epoch the
    loss, the early-stopper check BEFORE the loss is recorded and before the step, then the step.  ``evaluate(model) ->
    (loss, gradient)`` replaces ``model.loss_and_grad`` (a host evaluation drives the same loop without a device).
    ``likelihood="dirichlet"``: y holds integer labels and the model is a DirichletExactGP (``number_of_classes`` and
    ``fixed_noise`` go to it); the loss is then summed over the classes, as the reference's ``.sum()`` over the batch.
    ``kernel``: as the model classes take it, and also "periodic", "locally_periodic" and "trend_seasonal" (the model classes'
    ``kernel=PeriodicKernel``, ``kernel=LocallyPeriodicKernel`` and ``kernel=TrendSeasonalKernel``)."""
    set_seed(seed)
    kernel = _TRAINER_KERNEL_NAMES.get(kernel, kernel) if isinstance(kernel, str) else kernel
    if likelihood == "gaussian":
        model = ExactGP(x, y, kernel)
    elif likelihood == "dirichlet":
        model = DirichletExactGP(x, y, kernel, number_of_classes=number_of_classes, fixed_noise=fixed_noise)
    else:
        raise ValueError(f"train_exact_gp: likelihood must be 'gaussian' or 'dirichlet', got {likelihood!r}")
    evaluate = evaluate if evaluate is not None else type(model).loss_and_grad
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
    entries of ``state_dict()``, which are the raw values).  A DirichletExactGP holds one row of raw values per class: its
    rows are averaged first (the reference's ``mean(dim=0)`` over the batch), then the models.  Every block of the family's
    raw shape values (raw alpha, the raw period lengths, the raw periodic and seasonal lengthscales, the raw seasonal
    outputscale) is averaged like the raw lengthscales and the result is a kernel of the models' family."""
    first = models[0]
    per_model = [m.raw_parameters() for m in models]
    raw = torch.stack([r.mean(dim=0) if r.dim() == 2 else r for r in per_model]).mean(dim=0)
    blocks = [_repeated(_softplus(raw[columns]), first.d if per_dim else 1) for _, columns, per_dim in first._raw_blocks()]
    return first._make_kernel(blocks[0], float(_softplus(raw[2])), torch.cat(blocks[1:]) if blocks[1:] else raw[:0])


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
                    learning_rate: float, number_of_iterations: int, early_stopper_patience: float,
                    likelihood: str = "gaussian", number_of_classes: int | None = None,
                    subsample_fixed_noise: bool = True) -> List[ExactGP]:
    """runners.py:88-187 without its files and plots: ``number_of_iterations`` exact GPs, each on the ``subsample_size``
    neighbours of a point drawn under ``seed + i``; ONE on all of the data when the subsample covers it.
    ``likelihood="dirichlet"``: y holds integer labels; ``number_of_classes`` (default: ``y.max() + 1``) is taken from ALL
    of the data, because a subsample may lack a class.  ``subsample_fixed_noise=False`` trains a subsample that is smaller
    than the data without the fixed per-point noise, as the reference does (its likelihood is built on all N labels and
    gpytorch replaces a fixed noise of another length by zero)."""
    options = {}
    if likelihood == "dirichlet":
        classes = int(y.max()) + 1 if number_of_classes is None else int(number_of_classes)
        options = dict(likelihood=likelihood, number_of_classes=classes,
                       fixed_noise=bool(subsample_fixed_noise) or subsample_size >= x.shape[0])
    elif likelihood != "gaussian":
        raise ValueError(f"exact_gp_runner: likelihood must be 'gaussian' or 'dirichlet', got {likelihood!r}")
    if subsample_size >= x.shape[0]:
        number_of_iterations = 1
    models = []
    for i in range(number_of_iterations):
        set_seed(seed + i)
        centre = x[torch.randperm(x.shape[0])[0]]  # sample_point (src/samplers.py:47-62)
        xs, ys = nearest_subsample(x, y, subsample_size, centre)
        model, _ = train_exact_gp(xs, ys, kernel, seed, number_of_epochs, learning_rate, early_stopper_patience, **options)
        models.append(model)
    return models


__all__ = ["ExactGP", "SVGP", "DirichletExactGP", "dirichlet_targets", "softmax_normal_mean", "train_exact_gp", "construct_average_ard_kernel", "construct_average_gaussian_noise", "nearest_subsample",
           "exact_gp_runner", "NotPSDError", "fit_student_t", "estimate_student_parameters", "student_t_sums_on_device"]
