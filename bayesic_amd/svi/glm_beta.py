"""Beta regression (logit link) with a learned precision by reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_beta.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ Beta(a_n, b_n),  0 < y_n < 1,  a_n = m_n phi,  b_n = (1 - m_n) phi
        m_n = sigmoid(l_n),  l_n = x_n . w + o_n,  E y_n = m_n,  Var y_n = m_n (1 - m_n) / (1 + phi)
        w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0)
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The model for a proportion or a rate strictly inside (0, 1) -- a conversion rate per segment, the share of a budget
spent, a fraction defective, a loss given default.  A Gaussian fit of logit y estimates E logit y, a different mean, and
has the wrong variance law (svi/glm_gamma.py makes the same argument for log y).  The data enter one update through
ell_s, G_s (svi/glm.py) and T_s = d ell_s / d tau_s, all from ONE streaming pass over X (include/bayesic_hip.h,
bsc_glm_beta_data_pass); the precision draw tau_s rides with the weight draw w_s exactly as NegBinReparamSVI's dispersion
does, and the finish is that model's (the prior on e^tau has the same form).  step() = pass -> all-reduce of
[ell | G | T] -> bsc_glm_beta_update; the state, the first draw and step() are ReparamDriver's (svi/_reparam_base.py),
offsets and row weights svi/glm.py's (svi/_obs.py).  There is no ``exposure``: the link is a logit, and a multiplier on
a mean in (0, 1) is not a rate model -- pass offset=.  Weights are part of the likelihood and do not enter the mini-batch
scale.  The ELBO holds the full density: nothing is left out of ell.

y must be finite and strictly inside (0, 1) AFTER ROUNDING TO float32, the format the pass reads: a float64 0.99999999
rounds to 1.0f, where log1p(-y) is -infinity, and is refused.  It is checked where a batch is set -- the constructor and
set_batch, on the host before a device is asked for when y is a host array -- and never in step(); raw device pointers
are taken as they are.  The pass does not clamp.

Accuracy envelope of the pass: tau in [-2, 5] (phi from 0.135 to 148), |l| <= 80.

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more): no kernel of its own.

Limits, by design of this version: no random intercepts with this family (svi/hier_scalar.py has no HierBeta driver);
ReparamVI does not recognise a Beta log-joint; MiniBatchLoader does not carry offset and weights; there is no one-call
(pass + finish) form, so every update is pass -> all-reduce -> finish; no zero / one inflation -- a response with exact
zeros or ones is refused, not squeezed.  The multi-rank branch is wired like the other drivers' and has been exercised
at world size 1 only.
"""
import numpy as np

from ._scalar_latent import ScalarLatentDriver

RESPONSE_MSG = ("y must be finite and strictly inside (0, 1) after rounding to float32 (the response of a Beta model; "
                "a float64 value within 3e-8 of 1 rounds to 1.0f)")


def check_unit_interval(y):
    """y finite and 0 < y < 1 as float32 values (a host array, or a device tensor: one synchronisation, so it sits
    outside step())."""
    import torch
    if isinstance(y, torch.Tensor):
        a = y.to(torch.float32)
        ok = bool((torch.isfinite(a) & (a > 0) & (a < 1)).all())
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            a = np.asarray(y, np.float64).astype(np.float32)
        ok = bool(np.isfinite(a).all() and (a > 0).all() and (a < 1).all())
    if not ok:
        raise ValueError(RESPONSE_MSG)


class BetaReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: the constructor, set_batch, the phases, predict and the host views) with
    the precision phi = e^tau: ``a0``, ``b0`` are its Gamma(shape, rate) prior, tau = 0 at the default start is phi = 1,
    params() reports precision_mean = E_q[phi]."""
    link = "beta"
    pass_name, finish_name = "bsc_glm_beta_data_pass", "bsc_glm_beta_update"
    scalar_attr, mean_key, prior_noun = "_logprec", "precision_mean", "the precision"
    has_exposure = False
    check_response = staticmethod(check_unit_interval)

    @classmethod
    def check_arguments(cls, prior_precision, a0, b0, n_samples, offset=None, exposure=None):
        if exposure is not None:
            raise ValueError("exposure belongs to the Poisson rate model; the Beta model takes offset=")
        super().check_arguments(prior_precision, a0, b0, n_samples, offset, exposure)

    @property
    def logprec(self):
        return self._logprec[self.cur]


check_arguments = BetaReparamSVI.check_arguments
