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

Limits, by design of this version: no groups together with the dispersion; ReparamVI does not recognise a
negative-binomial log-joint; MiniBatchLoader does not carry offset and weights; there is no one-call (pass + finish)
form, so every update is pass -> all-reduce -> finish.  The multi-rank branch is wired like the other drivers' and has
been exercised at world size 1 only.
"""
import numpy as np

from ._obs import ObsBatch, batch_obs, check_link
from ._reparam_base import (ReparamDriver, check_covariance, check_lam0, check_n_samples, check_priors,
                            scalar_latent_covariance, scalar_latent_params)


def check_arguments(prior_precision, a0, b0, n_samples, offset, exposure):
    """The constructor's checks that need no device."""
    check_link("poisson", offset, exposure)      # a count model: exposure is allowed, not together with offset
    check_priors(prior_precision, a0, b0, "the dispersion")
    check_n_samples(n_samples)


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


class NegBinReparamSVI(ObsBatch, ReparamDriver):
    link = "negbin"          # svi/predict.py: family_of

    def __init__(self, X, y, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0, b0=0.1,
                 ctx=None, group=None, lam0=None, *, offset=None, weights=None, exposure=None, covariance="diag"):
        """``a0``, ``b0``: the Gamma(shape, rate) prior of the dispersion phi (default: mean 10, wide).  ``lam0``:
        [m | rho] over [w (D) | tau] (default m = 0 -- tau starts at 0, phi at 1 -- and every rho = log 0.1).
        ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the full
        layout, default the same start with no off-diagonal entries).
        ``offset`` / ``weights`` / ``exposure``: float32 [B], as in GLMReparamSVI.  y and the weights are checked here
        (finite, >= 0: one synchronisation), never in step()."""
        check_arguments(prior_precision, a0, b0, n_samples, offset, exposure)
        check_covariance(covariance)
        import torch
        host_y = not isinstance(y, torch.Tensor)
        if host_y:
            check_counts(y)                       # before a device is asked for
        shape = getattr(X, "shape", ())
        if len(shape) == 2:                       # an array or a tensor: lam0 too is checked before a device is asked for
            check_lam0(lam0, int(shape[1]) + 1, "w (%d) | tau" % int(shape[1]), covariance)
        from ..device import default_context
        self.covariance_kind = covariance
        self.prior_precision, self.a0, self.b0 = float(prior_precision), float(a0), float(b0)
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        if not host_y:
            check_counts(self.y)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        D, S = self.D, int(n_samples)
        P = D + 1
        check_lam0(lam0, P, "w (%d) | tau" % D, covariance)
        # stats = [ell | G | T]; the slab of the pass is 8 * 256 + 16 floats per workgroup
        self._init_state(P, lam0, n_total, S, seed, lr, group, noise_dim=D, w_cols=D, n_stats=S * (D + 2),
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 16) * 4)
        self.T = self.stats[S + S * D:]
        self._logphi = torch.zeros((2, S), dtype=torch.float32, device=self.ctx.device)

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None):
        """ReparamDriver.set_batch with the batch's offset and weights: tensors (y and the weights checked: finite,
        >= 0) with tensor X and y, raw device pointers (unchecked) with raw ones.  None drops the vector for this
        batch."""
        import torch
        if isinstance(X, torch.Tensor):
            check_counts(y)
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        super().set_batch(X, y, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)

    @property
    def logphi(self):
        return self._logphi[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def sample(self, step):
        """The first draw (first_draw) of w and tau, rounded to float32 as the finish rounds."""
        import torch
        z = self._first_draw(step).astype(np.float32)
        self._store_W(z, self.D)
        self._logphi[self.cur].copy_(torch.from_numpy(np.ascontiguousarray(z[:, self.D])))
        self._drawn = True

    def data_pass(self):
        self.ctx.call("bsc_glm_nb_data_pass", self._Xarg, self._ldx, self._yarg, self._oarg, self._varg, self.B, self.D,
                      self.W, self.logphi, self.S, self.ell, self.G, self.T)

    def _finish(self, stats):
        name = "bsc_glm_scalar_fullrank_update" if self.covariance_kind == "full" else "bsc_glm_nb_update"
        self._finish_latent(name, stats, self._logphi, (self.D,))

    # -- posterior predictive (svi/predict.py: one bsc_nb_predict_pass over X for all draws) -----------------------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
        from .predict import predict
        return predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                       weights=weights)

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
        """Mean log predictive density per held-out row (a host float); with weights sum v lpd / sum v."""
        from .predict import heldout_lpd
        return heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                           weights=weights)

    # -- host views -----------------------------------------------------------------------------------------------
    def params(self):
        """m and rho (host float64) whole and split -- w [D] and tau (scalars), each as (mean, rho) --, the dense
        lower-triangular L [P, P] of a full guide, and phi_mean = E_q[phi] = exp(m_tau + Var_q(tau) / 2) with Var_q(tau)
        = e^{2 rho_tau} (mean-field) or the squared norm of the last row of L (full)."""
        return scalar_latent_params(self.lam.cpu().numpy(), self.D, self.covariance_kind, "phi_mean")

    def covariance(self):
        """Cov_q over z = [w (D) | tau] (P x P, host float64): L L^T of the full guide, diag(e^{2 rho}) of the
        mean-field one."""
        return scalar_latent_covariance(self.lam.cpu().numpy(), self.D, self.covariance_kind)
