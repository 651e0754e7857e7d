"""Reparameterised-ELBO SVI for logistic and Poisson (log-link) regression on one fused pass.

Host-side driver of csrc/bsc_glm.hip; every numeric step is a C-ABI call into libbayesic_hip.so.  The reference
has no inference code -- this is README.md:51 (reparameterisation-trick gradient, refs [10][11][12]) with
mini-batch scaling per README.md:69-79 for the two canonical-link likelihoods that have no closed-form posterior.

Model:  y_n ~ Bernoulli(sigmoid(x_n . w))   or   y_n ~ Poisson(exp(x_n . w)),      w ~ N(0, I / prior_precision)
q:      w ~ N(m, diag e^{2 rho});  lam = [m (D) | rho (D)].

With l_ns = x_n . w_s the data enter one update only through ell_s = sum_n [y_n l_ns - A(l_ns)] and
G_s = sum_n (y_n - A'(l_ns)) x_n (A = softplus / exp): ONE streaming pass over X, y (bsc_glm_data_pass), then one
fused finish (bsc_glm_update: float64 reduction of the pass partials, ELBO, pathwise gradient with the analytic
entropy, Adam, the next step's draw) -- the shape of svi/blr.py, with lam and the draws double-buffered and the
noise drawn a block ahead by bsc_blr_noise (Philox stream 0, as oracle.svi.blr_sample; the layout's last column
belongs to BLR's scalar latent and is not read).  An intercept is a column of ones in X.  The ELBO of the Poisson
model leaves the constant -scale sum_n lnGamma(y_n + 1) out.

``covariance="full"``: q(w) = N(mu, L L^T), L lower-triangular with L_ii = e^{rho_i}; lam = [mu (D) | L packed
row-major, lower triangle incl. the diagonal (D(D+1)/2), rho_i in the diagonal slots] (include/bayesic_hip.h,
bsc_glm_fullrank_update: svi/blr.py's full layout with P = D).  The data pass is the same; the finish is
bsc_glm_fullrank_update, always behind data_pass() -> all_reduce(), so S up to 64 works and the exchange is the
mean-field driver's.  A mean-field guide cannot represent the posterior correlation of w that correlated features
induce and shrinks its marginal variances; the full guide can.

Offsets and row weights (``offset=``, ``weights=``, ``exposure=``): l_ns = x_n . w_s + o_n and every row's term of
ell_s and G_s times v_n >= 0 (include/bayesic_hip.h, bsc_glm_data_pass_obs; csrc/bsc_glm_obs.hip).  ``exposure`` is
the Poisson rate model's log E[y_n] = x_n . w + log exposure_n, kept as o = log(exposure).  Weights are part of the
likelihood (trials of aggregated binomial rows with y = k / n, survey weights, a mask of zeros) and do not enter the
mini-batch scale n_total / batch_rows.  A model built without them, and handed batches without them, calls the entry
points it always has.  The argument checks and the checked vectors of a batch are svi/_obs.py's, shared with
svi/hier_glm.py and svi/predict.py; the driver state, the first draw and the pass -> all-reduce -> finish step are
svi/_reparam_base.py's.

Data parallelism is wired as in svi/blr.py: each rank holds a block of mini-batch rows, and the one exchange per
update is an all-reduce(sum) of the float64 vector [ell (S) | G (S*D)] between the pass and the finish.  That branch
(the one every update of the full guide takes) has been exercised at world size 1 only.
"""
import torch

from ..device import default_context
from ._obs import LINKS, ObsBatch, batch_obs, check_link
from ._reparam_base import ReparamRegressionBase, full_size


class GLMReparamSVI(ObsBatch, ReparamRegressionBase):
    def __init__(self, X, y, link="logistic", n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0,
                 ctx=None, group=None, lam0=None, covariance="diag", *, offset=None, weights=None, exposure=None):
        """``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the
        full layout, default: the mean-field default's mu and rho with zero off-diagonal entries).
        ``offset`` / ``weights``: float32 [B], as y (module docstring); ``exposure``: Poisson only, strictly positive,
        instead of ``offset``.  The weights are checked here (finite, >= 0: one synchronisation), never in step()."""
        if covariance not in ("diag", "full"):
            raise ValueError("covariance must be 'diag' or 'full', got %r" % (covariance,))
        self.covariance_kind = covariance
        check_link(link, offset, exposure)
        self.link, self._link = link, LINKS[link]
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        self.prior_precision = float(prior_precision)
        if not self.prior_precision > 0.0:
            raise ValueError("prior_precision must be positive")
        D = self.D
        if lam0 is not None and covariance == "full" and torch.as_tensor(lam0).numel() != full_size(D):
            raise ValueError("lam0 has %d entries; covariance='full' at D = %d needs %d"
                             % (torch.as_tensor(lam0).numel(), D, full_size(D)))
        self._init_state(D, lam0, n_total, n_samples, seed, lr, group,
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 8) * 4)

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None):
        """ReparamDriver.set_batch with the batch's offset and weights: tensors (weights checked: finite, >= 0) with
        tensor X and y, raw device pointers (unchecked) with raw ones.  None drops the vector for this batch."""
        if isinstance(X, torch.Tensor):
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        super().set_batch(X, y, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)

    def data_pass(self):
        if self._oarg is None and self._varg is None:
            self.ctx.call("bsc_glm_data_pass", self._link, self._Xarg, self._ldx, self._yarg, self.B, self.D, self.W,
                          self.S, self.ell, self.G)
        else:
            self.ctx.call("bsc_glm_data_pass_obs", self._link, self._Xarg, self._ldx, self._yarg, self._oarg,
                          self._varg, self.B, self.D, self.W, self.S, self.ell, self.G)

    def _pass_update(self):
        """bsc_glm_pass_update[_obs]: the pass and the finish in one call; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1
        self._ensure_noise(t)
        state = (self._lam[c], self._lam[n], self.m1, self.m2, self._eps[self.t % self._ring], self._W[c], self.S)
        if self._oarg is None and self._varg is None:
            self.ctx.call("bsc_glm_pass_update", self._link, self._Xarg, self._ldx, self._yarg, self.B, self.D,
                          *state, *self._tail(t))
        else:
            self.ctx.call("bsc_glm_pass_update_obs", self._link, self._Xarg, self._ldx, self._yarg, self._oarg,
                          self._varg, self.B, self.D, *state, *self._tail(t))
        self.t = t

    def step(self):
        """One ELBO-gradient update; asynchronous on the context stream."""
        if self.world == 1 and not self.exchange.rccl and self.S <= 8 and self.covariance_kind == "diag":
            if not self._drawn:
                self.sample(self.t)  # Philox step index == number of completed updates
            self._pass_update()     # the pass and the finish in one call
        else:
            super().step()

    # -- posterior predictive (svi/predict.py: one bsc_predict_pass over X for all draws) --------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
        from .predict import predict
        return predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                       weights=weights)

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None, offset=None, exposure=None, weights=None):
        """Mean log predictive density per held-out row (a host float); with weights sum v lpd / sum v."""
        from .predict import heldout_lpd
        return heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                           weights=weights)

    # -- host views -----------------------------------------------------------
    def params(self):
        """diag: m, rho.  full: m = mu [D], the dense lower-triangular L [D, D] and rho = log diag L."""
        return self._flat_params()
