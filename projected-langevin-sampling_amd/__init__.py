"""MI355X-native projected Langevin sampling: the per-step particle update of
jswu18/projected-langevin-sampling behind the reference's PLS / basis / cost / link-function API.

All numerics run in libplship.so (hand-written HIP for gfx950, see csrc/); this package is the thin host
side: it owns device memory through torch tensors and calls the C ABI (include/plship.h) with raw pointers.
The one exception is the eigendecomposition of setup and prediction, torch.linalg.eigh by default as in the reference;
eigh_device="plship" runs it in the library as well (pls_sym_eigh)."""
from . import _lib
from .costs import BetaCost, GammaCost, NegativeBinomialCost, OrdinalCost
from .conformalise import ConformaliseGP, ConformalisePLS, ConformalPrediction, gaussian_interval
from .gaussian_process import (SVGP, DirichletExactGP, ExactGP, construct_average_ard_kernel, construct_average_gaussian_noise,
                               dirichlet_targets, estimate_student_parameters, exact_gp_runner, fit_student_t, nearest_subsample,
                               softmax_normal_mean, train_exact_gp)
from .kernel import (ARDKernel, LinearKernel, LocallyPeriodicKernel, MaternKernel, PeriodicKernel, PLSKernel, RQKernel,
                     TrendSeasonalKernel)
from .link_functions import ExponentialLinkFunction
from .likelihoods import BernoulliLikelihood, GaussianLikelihood, StudentTLikelihood
from .projected_langevin_sampling import PLS
from .runners import train_svgp_runner
from .temper import TemperGP
from .trainers import EarlyStopper, epoch_batches, train_pls, train_pls_captured, train_svgp

__all__ = ["PLS", "PLSKernel", "ARDKernel", "MaternKernel", "RQKernel", "PeriodicKernel", "LocallyPeriodicKernel", "TrendSeasonalKernel", "LinearKernel", "EarlyStopper", "train_pls", "train_pls_captured", "ExactGP",
           "DirichletExactGP", "dirichlet_targets", "softmax_normal_mean",
           "train_exact_gp", "exact_gp_runner", "construct_average_ard_kernel", "construct_average_gaussian_noise",
           "nearest_subsample", "SVGP", "train_svgp", "train_svgp_runner", "epoch_batches", "TemperGP", "GaussianLikelihood",
           "BernoulliLikelihood", "StudentTLikelihood", "fit_student_t", "estimate_student_parameters", "ConformaliseGP",
           "ConformalisePLS", "ConformalPrediction", "gaussian_interval", "NegativeBinomialCost", "ExponentialLinkFunction", "BetaCost",
           "OrdinalCost", "GammaCost", "_lib"]
