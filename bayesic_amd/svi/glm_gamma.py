"""Gamma regression (log link) with a learned shape by reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_gamma.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ Gamma(shape alpha, rate alpha / mu_n),  y_n > 0,  E y_n = mu_n = exp(l_n),  Var y_n = mu_n^2 / alpha
        l_n = x_n . w + o_n,   w ~ N(0, I / prior_precision),   alpha = e^tau ~ Gamma(a0, b0)
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The model for a positive, right-skewed, continuous response whose standard deviation grows with its mean (claim
severity, length of stay, time to failure, rainfall): the companion of the count models -- NegBinReparamSVI for how
many claims, this one for how large.  A Gaussian fit of log y estimates E log y, a different mean; a Poisson fit of
non-counts has the wrong variance law.  The data enter one update through ell_s, G_s (svi/glm.py) and T_s =
d ell_s / d tau_s, all from ONE streaming pass over X (include/bayesic_hip.h, bsc_glm_gamma_data_pass); the shape draw
tau_s rides with the weight draw w_s exactly as NegBinReparamSVI's dispersion does, and the finish is that model's
(the prior on e^tau has the same form).  step() = pass -> all-reduce of [ell | G | T] -> bsc_glm_gamma_update; the
state, the first draw and step() are ReparamDriver's (svi/_reparam_base.py), offsets, exposure and row weights
svi/glm.py's (svi/_obs.py): ``exposure`` is kept as o = log(exposure) (the log link makes E y proportional to it),
weights are part of the likelihood and do not enter the mini-batch scale.  The ELBO holds the full density: nothing is
left out of ell.

y must be finite and strictly positive.  It is checked where a batch is set -- the constructor and set_batch, on the
host before a device is asked for when y is a host array -- and never in step(); raw device pointers are taken as they
are.  The pass does not clamp: it is finite while y e^{-l} stays below the float32 maximum.

Accuracy envelope of the pass: tau in [-2.5, 5] (alpha from 0.08 to 148).

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more): the shape is correlated a posteriori with
the intercept, and a diagonal q reports it too narrow.

Random intercepts per group together with the shape: HierGammaReparamSVI (svi/hier_scalar.py).

Limits, by design of this version: ReparamVI does not recognise a Gamma log-joint; MiniBatchLoader does not carry
offset and weights; there is no one-call (pass + finish) form, so every update is pass -> all-reduce -> finish.  The
multi-rank branch is wired like the other drivers' and has been exercised at world size 1 only.
"""
import numpy as np

from ._scalar_latent import ScalarLatentDriver


def check_positive(y):
    """y finite and > 0 (a host array, or a device tensor: one synchronisation, so it sits outside step())."""
    import torch
    if isinstance(y, torch.Tensor):
        ok = bool((torch.isfinite(y) & (y > 0)).all())
    else:
        a = np.asarray(y, np.float64)
        ok = bool(np.isfinite(a).all() and (a > 0).all())
    if not ok:
        raise ValueError("y must be finite and > 0 (the response of a Gamma model)")


class GammaReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: the constructor, set_batch, the phases, predict and the host views) with
    the shape alpha = e^tau: ``a0``, ``b0`` are its Gamma(shape, rate) prior, tau = 0 at the default start is the
    exponential distribution, params() reports shape_mean = E_q[alpha]."""
    link = "gamma"
    pass_name, finish_name = "bsc_glm_gamma_data_pass", "bsc_glm_gamma_update"
    scalar_attr, mean_key, prior_noun = "_logshape", "shape_mean", "the shape"
    check_response = staticmethod(check_positive)

    @property
    def logshape(self):
        return self._logshape[self.cur]


check_arguments = GammaReparamSVI.check_arguments
