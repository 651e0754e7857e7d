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

Limits, by design of this version: no groups together with the shape; ReparamVI does not recognise a Gamma log-joint;
MiniBatchLoader does not carry offset and weights; there is no one-call (pass + finish) form, so every update is
pass -> all-reduce -> finish.  The multi-rank branch is wired like the other drivers' and has been exercised at world
size 1 only.
"""
import numpy as np

from ._obs import ObsBatch, batch_obs, check_link
from ._reparam_base import (ReparamDriver, check_covariance, check_lam0, check_n_samples, check_priors,
                            scalar_latent_covariance, scalar_latent_params)


def check_arguments(prior_precision, a0, b0, n_samples, offset, exposure):
    """The constructor's checks that need no device."""
    check_link("poisson", offset, exposure)      # a log link: exposure is allowed, not together with offset
    check_priors(prior_precision, a0, b0, "the shape")
    check_n_samples(n_samples)


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


class GammaReparamSVI(ObsBatch, ReparamDriver):
    link = "gamma"           # svi/predict.py: family_of

    def __init__(self, X, y, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0, b0=0.1,
                 ctx=None, group=None, lam0=None, *, offset=None, weights=None, exposure=None, covariance="diag"):
        """``a0``, ``b0``: the Gamma(shape, rate) prior of the shape alpha (default: mean 10, wide).  ``lam0``:
        [m | rho] over [w (D) | tau] (default m = 0 -- tau starts at 0, alpha at 1, the exponential distribution -- and
        every rho = log 0.1).  ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring;
        ``lam0`` then in the full layout, default the same start with no off-diagonal entries).  ``offset`` /
        ``weights`` / ``exposure``: float32 [B], as in GLMReparamSVI.  y and the weights are checked here (one
        synchronisation), never in step()."""
        check_arguments(prior_precision, a0, b0, n_samples, offset, exposure)
        check_covariance(covariance)
        import torch
        host_y = not isinstance(y, torch.Tensor)
        if host_y:
            check_positive(y)                     # before a device is asked for
        shape = getattr(X, "shape", ())
        if len(shape) == 2:                       # an array or a tensor: lam0 too is checked before a device is asked for
            check_lam0(lam0, int(shape[1]) + 1, "w (%d) | tau" % int(shape[1]), covariance)
        from ..device import default_context
        self.covariance_kind = covariance
        self.prior_precision, self.a0, self.b0 = float(prior_precision), float(a0), float(b0)
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        if not host_y:
            check_positive(self.y)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        D, S = self.D, int(n_samples)
        P = D + 1
        check_lam0(lam0, P, "w (%d) | tau" % D, covariance)
        # stats = [ell | G | T]; the slab of the pass is 8 * 256 + 16 floats per workgroup
        self._init_state(P, lam0, n_total, S, seed, lr, group, noise_dim=D, w_cols=D, n_stats=S * (D + 2),
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 16) * 4)
        self.T = self.stats[S + S * D:]
        self._logshape = torch.zeros((2, S), dtype=torch.float32, device=self.ctx.device)

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None):
        """ReparamDriver.set_batch with the batch's offset and weights: tensors (y checked finite and > 0, the weights
        finite and >= 0) with tensor X and y, raw device pointers (unchecked) with raw ones.  None drops the vector for
        this batch."""
        import torch
        if isinstance(X, torch.Tensor):
            check_positive(y)
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        super().set_batch(X, y, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)

    @property
    def logshape(self):
        return self._logshape[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def sample(self, step):
        """The first draw (first_draw) of w and tau, rounded to float32 as the finish rounds."""
        import torch
        z = self._first_draw(step).astype(np.float32)
        self._store_W(z, self.D)
        self._logshape[self.cur].copy_(torch.from_numpy(np.ascontiguousarray(z[:, self.D])))
        self._drawn = True

    def data_pass(self):
        self.ctx.call("bsc_glm_gamma_data_pass", self._Xarg, self._ldx, self._yarg, self._oarg, self._varg, self.B,
                      self.D, self.W, self.logshape, self.S, self.ell, self.G, self.T)

    def _finish(self, stats):
        name = "bsc_glm_scalar_fullrank_update" if self.covariance_kind == "full" else "bsc_glm_gamma_update"
        self._finish_latent(name, stats, self._logshape, (self.D,))

    # -- posterior predictive (svi/predict.py: one bsc_gamma_predict_pass over X for all draws) ---------------------
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
        lower-triangular L [P, P] of a full guide, and shape_mean = E_q[alpha] = exp(m_tau + Var_q(tau) / 2) with
        Var_q(tau) = e^{2 rho_tau} (mean-field) or the squared norm of the last row of L (full)."""
        return scalar_latent_params(self.lam.cpu().numpy(), self.D, self.covariance_kind, "shape_mean")

    def covariance(self):
        """Cov_q over z = [w (D) | tau] (P x P, host float64): L L^T of the full guide, diag(e^{2 rho}) of the
        mean-field one."""
        return scalar_latent_covariance(self.lam.cpu().numpy(), self.D, self.covariance_kind)
