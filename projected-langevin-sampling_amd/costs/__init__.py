from .base import PLSCost
from .bernoulli import BernoulliCost
from .beta import BetaCost
from .gamma import GammaCost
from .gaussian import GaussianCost
from .multimodal import MultiModalCost
from .negative_binomial import NegativeBinomialCost
from .ordinal import OrdinalCost
from .poisson import PoissonCost
from .student_t import StudentTCost

__all__ = ["PLSCost", "BernoulliCost", "GaussianCost", "PoissonCost", "StudentTCost", "MultiModalCost",
           "NegativeBinomialCost", "BetaCost", "OrdinalCost", "GammaCost"]
