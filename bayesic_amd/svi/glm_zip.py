"""Zero-inflated Poisson regression with a learned inflation odds by reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_zip.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ ZIP(pi, mu_n): with probability pi the row is a structural zero, otherwise y_n ~ Poisson(mu_n);
        mu_n = exp(l_n),   l_n = x_n . w + o_n,   w ~ N(0, I / prior_precision),
        omega = pi / (1 - pi) = e^tau ~ Gamma(a0, b0),   pi = sigmoid(tau).
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The count model for data with more zeros than a Poisson or a negative-binomial law allows (claims per policy, visits per
patient, defects per unit): a part of the population cannot produce a count at all.  A Poisson fit of such data pushes
its intercept down, a negative-binomial fit answers with a dispersion that stands for a different mechanism
(svi/glm_nb.py).  Here a zero enters through log(omega + e^{-mu}) - log1p(omega), a positive count through the Poisson
term minus log1p(omega) (include/bayesic_hip.h, bsc_glm_zip_data_pass); E y = (1 - pi) mu and
Var y = (1 - pi) mu (1 + pi mu).  One inflation share for all rows: there are no covariates on pi.

tau is the log ODDS of a structural zero, so that the prior on e^tau has the form the shared finish knows (``a0``,
``b0`` are the Gamma(shape, rate) prior of the odds) and the finish is NegBinReparamSVI's.  The default prior mean of
the odds is 1 (a0 = b0 = 1: a structural-zero share of one half, wide), NOT the other families' 10: an odds of ten
would say that 91 % of the rows are structural zeros.  The data enter one update through ell_s, G_s (svi/glm.py) and
T_s = d ell_s / d tau_s, all from ONE streaming pass over X; step() = pass -> all-reduce of [ell | G | T] ->
bsc_glm_zip_update; the state, the first draw and step() are ReparamDriver's (svi/_reparam_base.py); offsets, exposure
and row weights are svi/glm.py's (svi/_obs.py): ``exposure`` is kept as o = log(exposure) and scales the Poisson part's
mean.  The ELBO leaves the constant -scale sum_n v_n lnGamma(y_n + 1) out, as the Poisson model's does.

``y`` must be finite, >= 0 and whole.  It is checked where a batch is set -- the constructor and set_batch, on the host
before a device is asked for when it is a host array -- and never in step(); raw device pointers are taken as they are.
The pass does not clamp (like the Poisson pass): it is finite while e^l is.

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more): no kernel of its own.  The inflation odds
are correlated a posteriori with the intercept (more structural zeros, a higher Poisson mean); a diagonal q reports
both too narrow.

Out of scope, by design of this version: covariates on the zero share; the zero-inflated negative binomial (two learned
scalars); hurdle models; random intercepts (svi/hier_scalar.py has no driver for this family and predict(..., groups=)
refuses); recognition by ReparamVI; MiniBatchLoader (it does not carry offset and weights).  There is no one-call
(pass + finish) form, so every update is pass -> all-reduce -> finish.  The multi-rank branch is wired like the other
drivers' and has been exercised at world size 1 only.
"""
import math

import numpy as np

from ._scalar_latent import ScalarLatentDriver

GH_NODES = 64      # Gauss-Hermite nodes of zero_share_mean: within 1e-11 of the integral at sd(tau) <= 1.5, 3e-7 at sd = 3


def check_whole_counts(y):
    """y finite, >= 0 and whole (a host array, or a device tensor: one synchronisation, so it sits outside step())."""
    import torch
    if isinstance(y, torch.Tensor):
        ok = bool((torch.isfinite(y) & (y >= 0) & (y == torch.floor(y))).all())
    else:
        a = np.asarray(y, np.float64)
        ok = bool(np.isfinite(a).all() and (a >= 0).all() and (a == np.floor(a)).all())
    if not ok:
        raise ValueError("y must be finite, >= 0 and whole (counts of a zero-inflated Poisson model)")


def expected_sigmoid(mean, var):
    """E[sigmoid(tau)] for tau ~ N(mean, var), host float64, by Gauss-Hermite quadrature with GH_NODES nodes."""
    x, w = np.polynomial.hermite.hermgauss(GH_NODES)
    t = float(mean) + math.sqrt(2.0 * float(var)) * x
    e = np.exp(-np.abs(t))
    return float((w * np.where(t >= 0, 1.0, e) / (1.0 + e)).sum() / math.sqrt(math.pi))


class ZIPoissonReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: set_batch, the phases, predict and the host views) with the inflation
    odds omega = e^tau: ``a0``, ``b0`` are its Gamma(shape, rate) prior, params() reports odds_mean = E_q[omega] and
    zero_share_mean = E_q[sigmoid(tau)], the posterior mean share of structural zeros."""
    link = "zip"
    pass_name, finish_name = "bsc_glm_zip_data_pass", "bsc_glm_zip_update"
    scalar_attr, mean_key, prior_noun = "_logodds", "odds_mean", "the inflation odds"
    has_exposure = True
    check_response = staticmethod(check_whole_counts)

    def __init__(self, X, y, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0, b0=1.0,
                 ctx=None, group=None, lam0=None, *, offset=None, weights=None, exposure=None, covariance="diag"):
        """``y`` [B] finite, >= 0 and whole.  ``a0``, ``b0``: the Gamma(shape, rate) prior of the inflation odds
        pi / (1 - pi) -- default mean 1 (a zero share of one half), not the other families' 10, which would say 91 %
        structural zeros.  ``lam0``: [m | rho] over [w (D) | tau] (default m = 0 -- tau starts at 0, pi at 1/2 -- and
        every rho = log 0.1).  ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring;
        ``lam0`` then in the full layout).  ``offset`` / ``weights`` / ``exposure``: float32 [B], as in GLMReparamSVI.
        y and the weights are checked here (one synchronisation), never in step()."""
        self._construct(X, (y,), n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group, lam0, offset,
                        weights, exposure, covariance)

    @property
    def logodds(self):
        return self._logodds[self.cur]

    def zero_probability(self, X, n_samples=64, seed=None, draws=None, offset=None, exposure=None):
        """P(y_n = 0 | x_n) under the posterior predictive, float32 [B] on the device: one predictive pass at y = 0 (its
        lpd is the log of the draw average of pi + (1 - pi) e^{-mu}), exponentiated."""
        import torch
        from .predict import predict
        y = np.zeros(int(X.shape[0]), np.float32)
        return torch.exp(predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset,
                                 exposure=exposure)["lpd"])

    def params(self):
        """ScalarLatentDriver.params() -- odds_mean = E_q[e^tau] -- and zero_share_mean = E_q[sigmoid(tau)] by
        Gauss-Hermite quadrature in float64 on the host, with the marginal variance of tau under the full guide (the
        squared norm of the whole last row of L)."""
        out = super().params()
        D = self.D
        if self.covariance_kind == "full":
            var_tau = float((out["L"][D] ** 2).sum())
        else:
            var_tau = math.exp(2.0 * float(out["rho"][D]))
        out["zero_share_mean"] = expected_sigmoid(float(out["m"][D]), var_tau)
        return out


check_arguments = ZIPoissonReparamSVI.check_arguments
