"""Negative-binomial regression with a learned dispersion by reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_nb.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ NegBin(mean mu_n = exp(l_n), dispersion phi),   Var y_n = mu_n + mu_n^2 / phi,   l_n = x_n . w + o_n
        w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0)
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The count model for overdispersed rates (claims per policy-year, visits per patient, reads per gene): a Poisson fit of
such data returns posteriors that are too narrow and held-out scores that are too low, because its variance is tied to
its mean.  Here the data enter one update through ell_s, G_s (svi/glm.py) and T_s = d ell_s / d tau_s, all from ONE
streaming pass over X (include/bayesic_hip.h, bsc_glm_nb_data_pass): the dispersion draw tau_s rides with the weight
draw w_s, in the column of bsc_blr_noise's [S, D + 1] layout that belongs to a scalar latent.  step() = pass ->
all-reduce of [ell | G | T] -> bsc_glm_nb_update (ELBO, pathwise gradient, Adam, next draws); lam and the draws (W [S, D]
and logphi [S], both float32) are double-buffered, the first draw is made on the host.  The state, the first draw and
step() are ReparamDriver's (svi/_reparam_base.py); offsets, exposure and row weights are svi/glm.py's (svi/_obs.py):
``exposure`` is kept as o = log(exposure), weights are part of the likelihood and do not enter the mini-batch scale.
The ELBO leaves the constant -scale sum_n v_n lnGamma(y_n + 1) out, as the Poisson model's does.

Accuracy envelope of the pass: tau in [-2.5, 5] (phi from 0.08 to 148); above it the model is a Poisson model to the
precision of float32 and GLMReparamSVI(link="poisson") is the one to use.

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau], L lower-triangular with L_ii = e^{rho_i}; lam =
[mu (P) | L packed row-major, lower triangle incl. the diagonal] (svi/_reparam_base.py), the first draw is mu + L eps
and the finish is bsc_glm_scalar_fullrank_update, the one full-covariance finish of the three families with a learned
scalar (it sees [ell | G | T], never the likelihood).  The dispersion is correlated a posteriori with the intercept; a
diagonal q reports it too narrow.  The pass, the all-reduce, set_batch, offsets and weights are the same for both
guides.

Random intercepts per group together with the dispersion: HierNegBinReparamSVI (svi/hier_scalar.py).

Limits, by design of this version: ReparamVI does not recognise a negative-binomial log-joint; MiniBatchLoader does
not carry offset and weights; there is no one-call (pass + finish) form, so every update is pass -> all-reduce ->
finish.  The multi-rank branch is wired like the other drivers' and has been exercised at world size 1 only.
"""
import numpy as np

from ._scalar_latent import ScalarLatentDriver


def check_counts(y):
    """y finite and >= 0 (a host array, or a device tensor: one synchronisation, so it sits outside step())."""
    import torch
    if isinstance(y, torch.Tensor):
        ok = bool((torch.isfinite(y) & (y >= 0)).all())
    else:
        a = np.asarray(y, np.float64)
        ok = bool(np.isfinite(a).all() and (a >= 0).all())
    if not ok:
        raise ValueError("y must be finite and >= 0 (counts of a negative-binomial model)")


class NegBinReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: the constructor, set_batch, the phases, predict and the host views) with
    the dispersion phi = e^tau: ``a0``, ``b0`` are its Gamma(shape, rate) prior, params() reports phi_mean = E_q[phi]."""
    link = "negbin"
    pass_name, finish_name = "bsc_glm_nb_data_pass", "bsc_glm_nb_update"
    scalar_attr, mean_key, prior_noun = "_logphi", "phi_mean", "the dispersion"
    check_response = staticmethod(check_counts)

    @property
    def logphi(self):
        return self._logphi[self.cur]


check_arguments = NegBinReparamSVI.check_arguments
