"""Base kernels k and the PLS kernel r (drop-in for src/projected_langevin_sampling/kernel.py:5-79).

The reference takes a gpytorch kernel object; gpytorch is a host-side hyper-parameter container there.
Here kernels are plain parameter holders whose Gram matrices are built by libplship on the MI355X.
A gpytorch ScaleKernel(RBFKernel), ScaleKernel(MaternKernel), ScaleKernel(RQKernel), ScaleKernel(PeriodicKernel) or
ScaleKernel(RBFKernel * PeriodicKernel) instance, or the sum ScaleKernel(RBFKernel) + ScaleKernel(RBFKernel * PeriodicKernel), is
accepted wherever a base kernel is expected: its lengthscale / outputscale (and nu, alpha or period_length) are read once
(``as_base_kernel``)."""
from __future__ import annotations

import torch

from . import _lib as L


def _dev(x: torch.Tensor) -> torch.Tensor:
    """float64 contiguous copy on the current GPU (inputs may arrive as CPU / float32 tensors, as in the reference)."""
    if not torch.cuda.is_available():
        raise L.PlsHipError("no MI355X visible: the projected-Langevin hot path has no CPU fallback")
    return x.detach().to(device="cuda", dtype=torch.float64).contiguous()


class BaseKernel:
    """k(x1, x2) -> dense (n1, n2) float64 device tensor."""

    kind: int
    outputscale: float = 1.0

    @property
    def prior_variance(self) -> float:
        """k(x, x) of a stationary kernel, the same at every x: the outputscale, for a sum of scaled terms the sum of their
        outputscales.  (The linear kernel's k(x, x) depends on x: this value is not its diagonal.)"""
        return float(self.outputscale)

    def _lengthscale_dev(self, d: int) -> torch.Tensor | None:
        return None

    def __call__(self, x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        a, b = _dev(x1), _dev(x2)
        if a.dim() == 1:
            a = a[:, None]
        if b.dim() == 1:
            b = b[:, None]
        assert a.shape[1] == b.shape[1], "x1 and x2 must share the input dimension"
        n1, d = a.shape
        n2 = b.shape[0]
        out = torch.empty((n1, n2), dtype=torch.float64, device=a.device)
        ls = self._lengthscale_dev(d)
        L.check(
            L.load().pls_kernel_gram(
                self.kind, a.data_ptr(), n1, b.data_ptr(), n2, d, L.ptr(ls), float(self.outputscale), out.data_ptr(),
                max(n2, 1), L.stream_ptr(),
            ),
            "pls_kernel_gram",
        )
        return out

    forward = __call__


class _StationaryKernel(BaseKernel):
    """Holds per-dimension (or one shared) lengthscales and the outputscale; what the library reads is cached per D on the
    device.  A subclass declares its family: ``family`` is its name as the exact-GP classes and trainers take it,
    ``shape_blocks`` the ordered (attribute, per_dim) pairs of the shape values the library reads behind the d lengthscales,
    block after block (_lib.kernel_shape_params of them in all; empty: the family has none): the attribute that holds a
    block, which is also the constructor's argument for it, and whether it holds one value per dimension (or one shared by
    all), as the lengthscale does; ``keyword`` the constructor's argument beyond the lengthscale and the outputscale which a
    gpytorch kernel of the family carries as an attribute of the same name (None: ``as_base_kernel`` does not find the
    family that way)."""

    family: str
    keyword: str | None = None
    shape_blocks: tuple = ()

    def __init__(self, lengthscale, outputscale: float = 1.0):
        self.lengthscale = torch.as_tensor(lengthscale, dtype=torch.float64).reshape(-1).cpu()
        self.outputscale = float(outputscale)
        self._ls_dev: dict[int, torch.Tensor] = {}

    def _lengthscale_host(self, d: int) -> torch.Tensor:
        """the d + kernel_shape_params(kind, d) values the library reads: the lengthscales, then the shape blocks in their
        declared order (a value shared by all dimensions repeated per block)"""
        parts = []
        for name, per_dim in (("lengthscale", True),) + tuple(self.shape_blocks):
            v = torch.as_tensor(getattr(self, name), dtype=torch.float64).reshape(-1)
            if per_dim:
                v = v.expand(d) if v.numel() == 1 else v
                assert v.numel() == d, f"{name} has {v.numel()} entries, data has {d} dims"
            parts.append(v)
        return torch.cat(parts)

    def _lengthscale_dev(self, d: int) -> torch.Tensor:
        if d not in self._ls_dev:
            self._ls_dev[d] = _dev(self._lengthscale_host(d))
        return self._ls_dev[d]


class ARDKernel(_StationaryKernel):
    """ScaleKernel(RBFKernel(ard_num_dims=D)): k(a,b) = outputscale * exp(-0.5 sum_d ((a_d-b_d)/lengthscale_d)^2)
    (constructed in the reference at experiments/uci/regression/main.py:171-173, README.md:144-146)."""

    kind, family = L.KERNEL_RBF_ARD, "rbf"


class MaternKernel(_StationaryKernel):
    """ScaleKernel(MaternKernel(nu, ard_num_dims=D)): with r = |(a - b) / lengthscale| (per-dimension lengthscales),
    k(a,b) = outputscale * exp(-r)                              (nu = 1/2)
           = outputscale * (1 + sqrt3 r) exp(-sqrt3 r)           (nu = 3/2)
           = outputscale * (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r) (nu = 5/2),
    gpytorch's MaternKernel; nu is one of the three it offers.  Lengthscale handling as ARDKernel."""

    family, keyword = "matern", "nu"
    KINDS = {0.5: L.KERNEL_MATERN12, 1.5: L.KERNEL_MATERN32, 2.5: L.KERNEL_MATERN52}

    def __init__(self, lengthscale, outputscale: float = 1.0, nu: float = 2.5):
        nu = float(nu)
        if nu not in self.KINDS:
            raise ValueError(f"MaternKernel: nu must be 0.5, 1.5 or 2.5 (gpytorch's MaternKernel), got {nu}")
        super().__init__(lengthscale, outputscale)
        self.nu = nu
        self.kind = self.KINDS[nu]


class RQKernel(_StationaryKernel):
    """ScaleKernel(RQKernel(ard_num_dims=D)), the rational-quadratic kernel: with r^2 = sum_d ((a_d-b_d)/lengthscale_d)^2,
    k(a,b) = outputscale * (1 + r^2 / (2 alpha))^(-alpha),
    gpytorch's RQKernel as recalled (include/plship.h states the formula; it is the contract).  ``alpha`` > 0 is the shape:
    heavy tails for a small alpha, the RBF kernel as alpha -> inf.  ``lengthscale`` holds d (or one shared) values as in
    ARDKernel; the library reads alpha behind the lengthscales, so the device array has d + 1 entries."""

    kind, family = L.KERNEL_RQ, "rq"
    keyword, shape_blocks = "alpha", (("alpha", False),)

    def __init__(self, lengthscale, outputscale: float = 1.0, alpha: float = 1.0):
        alpha = float(torch.as_tensor(alpha, dtype=torch.float64).detach().reshape(-1)[0])  # (gpytorch's: a one-element tensor)
        if not alpha > 0.0:
            raise ValueError(f"RQKernel: alpha must be positive, got {alpha}")
        super().__init__(lengthscale, outputscale)
        self.alpha = alpha


class PeriodicKernel(_StationaryKernel):
    """ScaleKernel(PeriodicKernel(ard_num_dims=D)), the periodic kernel: with e_d = (a_d - b_d) / period_length_d,
    k(a,b) = outputscale * exp(-2 sum_d sin^2(pi e_d) / lengthscale_d),
    gpytorch's PeriodicKernel as recalled (include/plship.h states the formula; it is the contract): the lengthscale divides
    and is NOT squared -- MacKay's l^2 is this lengthscale.  ``lengthscale`` and ``period_length`` each hold d (or one
    shared) positive values; the library reads the period lengths behind the lengthscales, so the device array has 2 d
    entries.  d <= 16."""

    kind, family = L.KERNEL_PERIODIC, "periodic"
    keyword, shape_blocks = "period_length", (("period_length", True),)

    def __init__(self, lengthscale, outputscale: float = 1.0, period_length=1.0):
        period = torch.as_tensor(period_length, dtype=torch.float64).detach().reshape(-1).cpu()
        if period.numel() == 0 or not bool((period > 0.0).all()):
            raise ValueError(f"PeriodicKernel: every period length must be positive, got {period.tolist()}")
        super().__init__(lengthscale, outputscale)
        if not bool((self.lengthscale > 0.0).all()):
            raise ValueError(f"PeriodicKernel: every lengthscale must be positive, got {self.lengthscale.tolist()}")
        self.period_length = period


class LocallyPeriodicKernel(_StationaryKernel):
    """ScaleKernel(RBFKernel(ard_num_dims=D) * PeriodicKernel(ard_num_dims=D)), the locally periodic (quasi-periodic) kernel: a
    periodic kernel under an RBF envelope, so that the repeating shape may drift.  With e_d = (a_d - b_d) / period_length_d,
    k(a,b) = outputscale * exp(-(1/2 sum_d ((a_d - b_d) / lengthscale_d)^2 + 2 sum_d sin^2(pi e_d) / periodic_lengthscale_d)),
    gpytorch's product as recalled (include/plship.h states the formula; it is the contract).  ``lengthscale`` is the
    envelope's, ``periodic_lengthscale`` divides and is not squared, as PeriodicKernel's lengthscale.  Each of the three holds
    d (or one shared) positive values; the library reads them in that order, so the device array has 3 d entries.  d <= 16."""

    kind, family = L.KERNEL_LOCALLY_PERIODIC, "locally_periodic"
    shape_blocks = (("periodic_lengthscale", True), ("period_length", True))

    def __init__(self, lengthscale, outputscale: float = 1.0, periodic_lengthscale=1.0, period_length=1.0):
        super().__init__(lengthscale, outputscale)
        values = {"lengthscale": self.lengthscale}
        for name, given in (("periodic_lengthscale", periodic_lengthscale), ("period_length", period_length)):
            values[name] = torch.as_tensor(given, dtype=torch.float64).detach().reshape(-1).cpu()
        for name, v in values.items():
            if v.numel() == 0 or not bool((v > 0.0).all()):
                raise ValueError(f"LocallyPeriodicKernel: every {name.replace('_', ' ')} must be positive, got {v.tolist()}")
        self.periodic_lengthscale, self.period_length = values["periodic_lengthscale"], values["period_length"]


class TrendSeasonalKernel(_StationaryKernel):
    """ScaleKernel(RBFKernel(ard_num_dims=D)) + ScaleKernel(RBFKernel(ard_num_dims=D) * PeriodicKernel(ard_num_dims=D)): a slow
    trend added to a locally periodic seasonal part.  With e_d = (a_d - b_d) / period_length_d,
    k(a,b) = outputscale * exp(-1/2 sum_d ((a_d - b_d) / lengthscale_d)^2)
           + seasonal_outputscale * exp(-(1/2 sum_d ((a_d - b_d) / seasonal_lengthscale_d)^2
                                          + 2 sum_d sin^2(pi e_d) / periodic_lengthscale_d)),
    gpytorch's sum as recalled (include/plship.h states the formula; it is the contract).  ``lengthscale`` and ``outputscale``
    are the trend's; ``seasonal_lengthscale`` is the envelope of the seasonal term, ``periodic_lengthscale`` divides and is not
    squared, as PeriodicKernel's lengthscale.  Each of the four per-dimension blocks holds d (or one shared) positive values;
    the library reads them in that order and the seasonal outputscale behind them, so the device array has 4 d + 1 entries.
    k(x, x) = outputscale + seasonal_outputscale (``prior_variance``).  d <= 8."""

    kind, family = L.KERNEL_TREND_SEASONAL, "trend_seasonal"
    shape_blocks = (("seasonal_lengthscale", True), ("periodic_lengthscale", True), ("period_length", True),
                    ("seasonal_outputscale", False))

    def __init__(self, lengthscale, outputscale: float = 1.0, seasonal_lengthscale=1.0, periodic_lengthscale=1.0,
                 period_length=1.0, seasonal_outputscale: float = 1.0):
        super().__init__(lengthscale, outputscale)
        values = {"lengthscale": self.lengthscale}  # (the trend's outputscale is as free as every family's)
        for name, given in (("seasonal_lengthscale", seasonal_lengthscale), ("periodic_lengthscale", periodic_lengthscale),
                            ("period_length", period_length), ("seasonal_outputscale", seasonal_outputscale)):
            values[name] = torch.as_tensor(given, dtype=torch.float64).detach().reshape(-1).cpu()
        for name, v in values.items():
            if v.numel() == 0 or not bool((v > 0.0).all()):
                raise ValueError(f"TrendSeasonalKernel: every {name.replace('_', ' ')} must be positive, got {v.tolist()}")
        self.seasonal_lengthscale, self.periodic_lengthscale = values["seasonal_lengthscale"], values["periodic_lengthscale"]
        self.period_length = values["period_length"]
        self.seasonal_outputscale = float(values["seasonal_outputscale"][0])  # (a one-element tensor is taken as its value)

    @property
    def prior_variance(self) -> float:
        return self.outputscale + self.seasonal_outputscale


class LinearKernel(BaseKernel):
    """k(x1, x2) = x1 x2^T: the reference's test double (mockers/kernel.py:8-23)."""

    kind = L.KERNEL_LINEAR


#: the stationary families, in the order ``as_base_kernel`` asks a gpytorch kernel for their keywords: nu, alpha, period_length
STATIONARY_KERNELS = (ARDKernel, MaternKernel, RQKernel, PeriodicKernel, LocallyPeriodicKernel, TrendSeasonalKernel)
#: "ARDKernel / MaternKernel / RQKernel / PeriodicKernel / LocallyPeriodicKernel / TrendSeasonalKernel", as the error messages of the package list them
STATIONARY_KERNEL_NAMES = " / ".join(cls.__name__ for cls in STATIONARY_KERNELS)


def as_base_kernel(kernel) -> BaseKernel:
    """Accept our kernels, or read the hyper-parameters of a gpytorch ScaleKernel(RBFKernel), ScaleKernel(MaternKernel) (an
    inner kernel with a ``nu`` attribute; nu outside {0.5, 1.5, 2.5} raises ValueError), ScaleKernel(RQKernel) (an inner
    kernel with an ``alpha`` attribute), ScaleKernel(PeriodicKernel) (an inner kernel with a ``period_length`` attribute) or
    ScaleKernel(RBFKernel * PeriodicKernel) (gpytorch's product as recalled: an inner kernel with a ``kernels`` sequence of
    two members that both have a ``lengthscale``, exactly one of them a ``period_length``; the other, which must have none of
    ``nu``, ``alpha`` and ``period_length``, is the envelope).  One sum is read as well, gpytorch's as recalled:
    ScaleKernel(RBFKernel) + ScaleKernel(RBFKernel * PeriodicKernel) -- an object without a ``base_kernel`` whose ``kernels``
    sequence has exactly two members, each with a ``base_kernel`` and an ``outputscale``, of which one reads as an ARDKernel
    and the other as a LocallyPeriodicKernel by the rules above, in either order; every other sum raises TypeError."""
    if isinstance(kernel, BaseKernel):
        return kernel
    terms = getattr(kernel, "kernels", None)
    if terms is not None and not hasattr(kernel, "base_kernel"):
        terms = list(terms)
        if len(terms) == 2 and all(hasattr(m, "base_kernel") and hasattr(m, "outputscale") for m in terms):
            try:
                read = [as_base_kernel(m) for m in terms]
            except TypeError:
                read = []
            trend = [k for k in read if type(k) is ARDKernel]
            seasonal = [k for k in read if type(k) is LocallyPeriodicKernel]
            if len(trend) == len(seasonal) == 1:
                trend, seasonal = trend[0], seasonal[0]
                return TrendSeasonalKernel(lengthscale=trend.lengthscale, outputscale=trend.outputscale,
                                           seasonal_lengthscale=seasonal.lengthscale, periodic_lengthscale=seasonal.periodic_lengthscale,
                                           period_length=seasonal.period_length, seasonal_outputscale=seasonal.outputscale)
        raise TypeError(f"unsupported base kernel {type(kernel).__name__}: use {STATIONARY_KERNEL_NAMES} / LinearKernel")
    inner = getattr(kernel, "base_kernel", None)
    members = getattr(inner, "kernels", None)
    if members is not None and hasattr(kernel, "outputscale"):
        members = list(members)
        periodic = [m for m in members if hasattr(m, "period_length")]
        envelope = [m for m in members if not any(hasattr(m, cls.keyword) for cls in STATIONARY_KERNELS if cls.keyword)]  # (no nu, alpha, period_length: RBF)
        if len(members) == 2 and len(periodic) == len(envelope) == 1 and all(getattr(m, "lengthscale", None) is not None for m in members):
            envelope = envelope[0]
            flat = lambda v: torch.as_tensor(v).detach().reshape(-1)  # noqa: E731
            return LocallyPeriodicKernel(lengthscale=flat(envelope.lengthscale), outputscale=float(torch.as_tensor(kernel.outputscale).detach()),
                                         periodic_lengthscale=flat(periodic[0].lengthscale), period_length=flat(periodic[0].period_length))
    elif inner is not None and hasattr(inner, "lengthscale") and hasattr(kernel, "outputscale"):
        lengthscale = torch.as_tensor(inner.lengthscale).detach().reshape(-1)
        outputscale = float(torch.as_tensor(kernel.outputscale).detach())
        for cls in STATIONARY_KERNELS:
            if cls.keyword is not None and hasattr(inner, cls.keyword):
                return cls(lengthscale=lengthscale, outputscale=outputscale, **{cls.keyword: getattr(inner, cls.keyword)})
        return ARDKernel(lengthscale=lengthscale, outputscale=outputscale)
    raise TypeError(f"unsupported base kernel {type(kernel).__name__}: use {STATIONARY_KERNEL_NAMES} / LinearKernel")


class PLSKernel:
    """r(x1, x2) = (1/n_S) k(x1, S) k(x2, S)^T over the unique approximation samples S (kernel.py:31-76)."""

    def __init__(self, base_kernel, approximation_samples: torch.Tensor, **kwargs):
        self.base_kernel = as_base_kernel(base_kernel)
        self.approximation_samples = approximation_samples

    def forward(
        self,
        x1: torch.Tensor,
        x2: torch.Tensor,
        additional_approximation_samples: torch.Tensor | None = None,
        last_dim_is_batch: bool = False,
        diag: bool = False,
        **params,
    ) -> torch.Tensor:
        samples = [self.approximation_samples.detach().cpu().to(torch.float64)]
        if additional_approximation_samples is not None:
            samples.append(additional_approximation_samples.detach().cpu().to(torch.float64))
        s = torch.cat([t if t.dim() == 2 else t[:, None] for t in samples], dim=0).unique(dim=0)  # kernel.py:43-45
        n_s = s.shape[0]
        g1 = self.base_kernel(s, x1)  # k(S, x1)  (n_S, n1): k-major operand
        g2 = self.base_kernel(s, x2)  # k(S, x2)  (n_S, n2)
        n1, n2 = g1.shape[1], g2.shape[1]
        res = torch.empty((n1, n2), dtype=torch.float64, device=g1.device)
        L.check(
            L.load().pls_gemm_tn(
                g1.data_ptr(), L.ld(g1), g2.data_ptr(), L.ld(g2), res.data_ptr(), max(n2, 1), n1, n2, n_s, 1.0 / n_s, 0.0,
                L.stream_ptr(),
            ),
            "pls_gemm_tn",
        )
        return res.diag() if diag else res

    __call__ = forward
