"""Student-t robust regression with a learned scale and fixed degrees of freedom by reparameterised-ELBO SVI on the fused
pass.

Host-side driver of csrc/bsc_glm_studentt.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ StudentT(df = nu, location l_n, scale sigma),   l_n = x_n . w + o_n,   w ~ N(0, I / prior_precision),
        k = 1 / sigma = e^tau ~ Gamma(a0, b0);   nu > 0 is fixed by the user (``df``, default 4).
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The model for a real-valued response with noise of unknown size and the occasional gross error (a mistyped figure, a
sensor that stuck, a trade booked twice).  Under the Gaussian likelihood (BLRReparamSVI) the pull of a row on the fit
grows with its residual without limit, and one outlier moves the coefficients as far as it likes.  Here a row enters
through log p = tau + c_nu - ((nu + 1) / 2) log1p(z^2 / nu), z = k (y - l), whose derivative in l,
k (nu + 1) z / (nu + z^2), is BOUNDED: it grows up to |z| = sqrt(nu) and falls like 1 / z beyond, so a row that is far
out is all but ignored.  nu sets where that happens: 4 (the default) is a common choice for robustness, 1 is the Cauchy
distribution, 30 is close to the Gaussian and 1e6 is the Gaussian to six digits.  l is the LOCATION: the mean of y for
nu > 1 and its median for every nu; Var y = nu sigma^2 / (nu - 2) for nu > 2 and infinite otherwise, and predict()
reports ``var`` = +inf then.

tau is the log of the INVERSE scale, not of sigma, as in LogNormalReparamSVI (svi/glm_lognormal.py): the prior on e^tau
then has the form the shared finish knows (``a0``, ``b0`` are the Gamma(shape, rate) prior of 1 / sigma), and the finish
is NegBinReparamSVI's; it never sees nu.  The data enter one update through ell_s, G_s (svi/glm.py) and
T_s = d ell_s / d tau_s, all from ONE streaming pass over X; step() = pass -> all-reduce of [ell | G | T] ->
bsc_glm_studentt_update; the state, the first draw and step() are ReparamDriver's (svi/_reparam_base.py), offsets and
row weights svi/glm.py's (svi/_obs.py).  nu is a constant of the MODEL and goes to the pass, and to the predictive pass,
as one argument of each call (include/bayesic_hip.h, bsc_glm_studentt_data_pass); the device takes it rounded to
float32.  There is no ``exposure``: the link is the identity, and ``offset`` is the known part of the location.

``y`` must be finite.  It is checked where a batch is set -- the constructor and set_batch, on the host before a device
is asked for when it is a host array -- and never in step(); raw device pointers are taken as they are.  ``df`` is
checked in the constructor: finite and > 0.  The pass does not clamp and has nothing to clamp: every term is finite
while z^2 is.

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more): no kernel of its own.

Out of scope, by design of this version: a learned nu (it is a constant here; compare fits at several values by
heldout_lpd); random intercepts (svi/hier_scalar.py has no driver for this family and predict(..., groups=) refuses);
recognition by ReparamVI (it does not recognise a Student-t log-joint); MiniBatchLoader (it does not carry offset and
weights).  There is no one-call (pass + finish) form, so every update is pass -> all-reduce -> finish.  The multi-rank
branch is wired like the other drivers' and has been exercised at world size 1 only.
"""
import math

import numpy as np

from ._scalar_latent import ScalarLatentDriver

Y_MSG = "y must be finite (a real-valued response; drop a missing row or give it weight 0)"
DF_MSG = "df=%r must be a finite number > 0 (the degrees of freedom of the Student-t likelihood; 1e6 is the Gaussian)"


def check_finite(y):
    """y finite (a host array, or a device tensor: one synchronisation, so it sits outside step())."""
    import torch
    if isinstance(y, torch.Tensor):
        ok = bool(torch.isfinite(y).all())
    else:
        with np.errstate(over="ignore"):
            ok = bool(np.isfinite(np.asarray(y, np.float32)).all())      # as the device reads it
    if not ok:
        raise ValueError(Y_MSG)


def check_df(df):
    """``df`` as a host float: finite, > 0 and a normal float32 once rounded, which is what the kernels take."""
    try:
        nu = float(df)
    except (TypeError, ValueError):
        raise ValueError(DF_MSG % (df,)) from None
    with np.errstate(over="ignore"):
        nu32 = float(np.float32(nu))
    if not (math.isfinite(nu) and nu > 0.0 and math.isfinite(nu32) and nu32 >= float(np.finfo(np.float32).tiny)):
        raise ValueError(DF_MSG % (df,))
    return nu


class StudentTReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: set_batch, the phases and the host views) with the inverse scale
    k = 1 / sigma = e^tau and the degrees of freedom ``df``, which every pass is handed; params() reports
    inv_sigma_mean = E_q[1 / sigma], sigma_mean = E_q[sigma] and df."""
    link = "studentt"
    pass_name, finish_name = "bsc_glm_studentt_data_pass", "bsc_glm_studentt_update"
    scalar_attr, mean_key, prior_noun = "_loginvscale", "inv_sigma_mean", "the inverse scale"
    has_exposure = False
    check_response = staticmethod(check_finite)

    def __init__(self, X, y, df=4.0, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0, b0=0.1,
                 ctx=None, group=None, lam0=None, *, offset=None, weights=None, covariance="diag"):
        """``y`` [B] finite.  ``df``: the degrees of freedom nu, finite and > 0 (module docstring), fixed for the life of
        the model.  ``a0``, ``b0``: the Gamma(shape, rate) prior of the inverse scale 1 / sigma (default: mean 10,
        wide).  ``lam0``: [m | rho] over [w (D) | tau] (default m = 0 -- tau starts at 0, sigma at 1 -- and every
        rho = log 0.1).  ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0``
        then in the full layout).  ``offset`` / ``weights``: float32 [B], as in GLMReparamSVI.  df, y and the weights
        are checked here (one synchronisation), never in step()."""
        self.df = check_df(df)
        self._construct(X, (y,), n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group, lam0, offset,
                        weights, None, covariance)

    @property
    def loginvscale(self):
        return self._loginvscale[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def data_pass(self):
        # the one pass that takes a constant of the model: df behind S
        self.ctx.call(self.pass_name, self._Xarg, self._ldx, self._yarg, self._oarg, self._varg, self.B, self.D, self.W,
                      self.loginvscale, self.S, self.df, self.ell, self.G, self.T)

    # -- posterior predictive (svi/predict.py: one bsc_studentt_predict_pass over X for all draws) ------------------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """``mean`` = the posterior-predictive average of the LOCATION per row (the mean of y for df > 1, its median
        always) and ``var`` (+inf for df <= 2) and, with ``y``, ``lpd`` and ``lpd_sum``."""
        from .predict import predict
        return predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights)

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """Mean log predictive density per held-out row (a host float); with weights sum v lpd / sum v."""
        from .predict import heldout_lpd
        return heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights)

    # -- host views -----------------------------------------------------------------------------------------------
    def params(self):
        """ScalarLatentDriver.params() -- inv_sigma_mean = E_q[e^tau] = exp(m_tau + Var_q(tau) / 2) --, sigma_mean =
        E_q[e^{-tau}] = exp(-m_tau + Var_q(tau) / 2), with the marginal variance of tau under the full guide, and df."""
        out = super().params()
        out["sigma_mean"] = out["inv_sigma_mean"] * math.exp(-2.0 * float(out["tau"][0]))
        out["df"] = self.df
        return out


check_arguments = StudentTReparamSVI.check_arguments
