"""Host-side drivers of the SVI inner loop (one class per BASELINE config)."""

from .glm import GLMReparamSVI  # noqa: E402,F401
from .glm_beta import BetaReparamSVI  # noqa: E402,F401
from .glm_gamma import GammaReparamSVI  # noqa: E402,F401
from .glm_lognormal import LogNormalReparamSVI  # noqa: E402,F401
from .glm_nb import NegBinReparamSVI  # noqa: E402,F401
from .glm_ordinal import OrdinalReparamSVI  # noqa: E402,F401
from .glm_studentt import StudentTReparamSVI  # noqa: E402,F401
from .glm_weibull import WeibullReparamSVI  # noqa: E402,F401
from .glm_zip import ZIPoissonReparamSVI  # noqa: E402,F401
from .hier_glm import HierGLMReparamSVI  # noqa: E402,F401
from .hier_scalar import HierGammaReparamSVI, HierNegBinReparamSVI, HierWeibullReparamSVI  # noqa: E402,F401
from .softmax import SoftmaxReparamSVI  # noqa: E402,F401
from . import predict  # noqa: E402,F401  (the module: predict.predict(model, X, ...))
from .predict import heldout_lpd, posterior_draws  # noqa: E402,F401

__all__ = ["BetaReparamSVI", "GLMReparamSVI", "GammaReparamSVI", "HierGLMReparamSVI", "HierGammaReparamSVI",
           "HierNegBinReparamSVI", "HierWeibullReparamSVI", "LogNormalReparamSVI", "NegBinReparamSVI",
           "OrdinalReparamSVI", "SoftmaxReparamSVI", "StudentTReparamSVI", "WeibullReparamSVI", "ZIPoissonReparamSVI",
           "predict", "posterior_draws", "heldout_lpd"]
