"""What the drivers with ONE learned log-scalar behind the weights share (svi/glm_nb.py, svi/glm_gamma.py,
svi/glm_weibull.py): q over z = [w (D) | tau], e^tau ~ Gamma(a0, b0) the family's dispersion or shape.

The device side is one kernel set (csrc/bsc_scalar_family.h) behind three entry points per family -- the data pass, the
mean-field finish, the predictive pass -- and bsc_glm_scalar_fullrank_update for ``covariance="full"``; this is the host
side of all of them.  A family states, as class attributes,

    link          svi/predict.py's name of the family (family_of)
    pass_name     its data pass, bsc_glm_*_data_pass
    finish_name   its mean-field finish, bsc_glm_*_update
    scalar_attr   the attribute of the [2, S] float32 double buffer of the tau draws ("_logphi", "_logshape")
    mean_key      the key of E_q[e^tau] in params() ("phi_mean", "shape_mean")
    prior_noun    what check_priors calls e^tau ("the dispersion", "the shape")
    has_exposure  whether ``exposure`` exists (a log link for a mean: yes; a log scale: no)

and ``check_response``, the check of y where a batch is set (finite and >= 0, finite and > 0).  A family whose response
is more than one checked vector (Weibull: time, event, upper) hands the tuple to _construct and overrides
_checked_response and _set_response, which take it, instead (and set_batch, the one user of check_response besides
them).
"""
import numpy as np

from ._obs import ObsBatch, batch_obs, check_link
from ._reparam_base import (ReparamDriver, check_covariance, check_lam0, check_n_samples, check_priors,
                            scalar_latent_covariance, scalar_latent_params)


class ScalarLatentDriver(ObsBatch, ReparamDriver):
    has_exposure = True

    @classmethod
    def check_arguments(cls, prior_precision, a0, b0, n_samples, offset=None, exposure=None):
        """The constructor's checks that need no device."""
        if cls.has_exposure:
            check_link("poisson", offset, exposure)      # a log link: exposure is allowed, not together with offset
        check_priors(prior_precision, a0, b0, cls.prior_noun)
        check_n_samples(n_samples)

    def __init__(self, X, y, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0, b0=0.1,
                 ctx=None, group=None, lam0=None, *, offset=None, weights=None, exposure=None, covariance="diag"):
        """``a0``, ``b0``: the Gamma(shape, rate) prior of e^tau (default: mean 10, wide).  ``lam0``: [m | rho] over
        [w (D) | tau] (default m = 0 -- tau starts at 0, e^tau at 1 -- and every rho = log 0.1).  ``covariance``: "diag"
        (the mean-field guide, default) or "full" (the family's module docstring; ``lam0`` then in the full layout,
        default the same start with no off-diagonal entries).  ``offset`` / ``weights`` / ``exposure``: float32 [B], as
        in GLMReparamSVI.  The response and the weights are checked here (one synchronisation), never in step()."""
        self._construct(X, (y,), n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group, lam0, offset,
                        weights, exposure, covariance)

    def _construct(self, X, response, n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group, lam0, offset,
                   weights, exposure, covariance):
        """The constructor; ``response``: the tuple of vectors the family's two response hooks take, y first."""
        self.check_arguments(prior_precision, a0, b0, n_samples, offset, exposure)
        check_covariance(covariance)
        import torch
        host = not isinstance(response[0], torch.Tensor)
        checked = self._checked_response(*response) if host else None     # before a device is asked for
        shape = getattr(X, "shape", ())
        if len(shape) == 2:                       # an array or a tensor: lam0 too is checked before a device is asked for
            check_lam0(lam0, int(shape[1]) + 1, "w (%d) | tau" % int(shape[1]), covariance)
        from ..device import default_context
        self.covariance_kind = covariance
        self.prior_precision, self.a0, self.b0 = float(prior_precision), float(a0), float(b0)
        self.ctx = ctx or default_context()
        self._set_response(X, response, checked)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        D, S = self.D, int(n_samples)
        P = D + 1
        check_lam0(lam0, P, "w (%d) | tau" % D, covariance)
        # stats = [ell | G | T]; the slab of the pass is 8 * 256 + 16 floats per workgroup
        self._init_state(P, lam0, n_total, S, seed, lr, group, noise_dim=D, w_cols=D, n_stats=S * (D + 2),
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 16) * 4)
        self.T = self.stats[S + S * D:]
        setattr(self, self.scalar_attr, torch.zeros((2, S), dtype=torch.float32, device=self.ctx.device))

    def _checked_response(self, y):
        """A host response, checked: what _set_response gets as ``checked``."""
        self.check_response(y)
        return y

    def _set_response(self, X, response, checked):
        """The constructor's batch.  ``checked``: what _checked_response made of a host response, None for tensors,
        which are checked here, once their dtype and shape are known to be right."""
        self._float_batch(X, response[0])
        if checked is None:
            self.check_response(self.y)

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None):
        """ReparamDriver.set_batch with the batch's offset and weights: tensors (y checked as in the constructor, the
        weights finite and >= 0) with tensor X and y, raw device pointers (unchecked) with raw ones.  None drops the
        vector for this batch."""
        import torch
        if isinstance(X, torch.Tensor):
            self.check_response(y)
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        super().set_batch(X, y, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)

    @property
    def _scalar(self):
        """The [2, S] double buffer of the tau draws."""
        return getattr(self, self.scalar_attr)

    # -- phases -------------------------------------------------------------------------------------------------
    def sample(self, step):
        """The first draw (first_draw) of w and tau, rounded to float32 as the finish rounds."""
        import torch
        z = self._first_draw(step).astype(np.float32)
        self._store_W(z, self.D)
        self._scalar[self.cur].copy_(torch.from_numpy(np.ascontiguousarray(z[:, self.D])))
        self._drawn = True

    def data_pass(self):
        self.ctx.call(self.pass_name, self._Xarg, self._ldx, self._yarg, self._oarg, self._varg, self.B, self.D, self.W,
                      self._scalar[self.cur], self.S, self.ell, self.G, self.T)

    def _finish(self, stats):
        name = "bsc_glm_scalar_fullrank_update" if self.covariance_kind == "full" else self.finish_name
        self._finish_latent(name, stats, self._scalar, (self.D,))

    # -- posterior predictive (svi/predict.py: one predictive pass over X for all draws) ----------------------------
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
        lower-triangular L [P, P] of a full guide, and ``mean_key`` = E_q[e^tau] = exp(m_tau + Var_q(tau) / 2) with
        Var_q(tau) = e^{2 rho_tau} (mean-field) or the squared norm of the last row of L (full)."""
        return scalar_latent_params(self.lam.cpu().numpy(), self.D, self.covariance_kind, self.mean_key)

    def covariance(self):
        """Cov_q over z = [w (D) | tau] (P x P, host float64): L L^T of the full guide, diag(e^{2 rho}) of the
        mean-field one."""
        return scalar_latent_covariance(self.lam.cpu().numpy(), self.D, self.covariance_kind)
