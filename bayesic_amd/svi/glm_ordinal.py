"""Ordinal (cumulative-logit, proportional-odds) regression with learned cutpoints by reparameterised-ELBO SVI on the
fused pass.

Host-side driver of csrc/bsc_glm_ordinal.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n in {0 .. K-1}, ORDERED (Likert items, severity grades, star ratings, credit bands), 2 <= K <= 8;
        eta_n = x_n . w + o_n,   cutpoints c_0 < .. < c_{K-2}:
        P(y_n <= k) = sigmoid(c_k - eta_n),   P(y_n = k) = sigmoid(c_k - eta_n) - sigmoid(c_{k-1} - eta_n)
        theta_0 = c_0,  theta_j = log(c_j - c_{j-1})  (j >= 1):  every draw is ordered by construction
        z = [w (D) | theta (K - 1)] ~ N(0, I / prior_precision),   P = D + K - 1
q:      z ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)]                         (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                               (covariance="full", below).

THERE IS NO INTERCEPT COLUMN: the cutpoints are the intercepts (a column of ones in X is not identified against them;
the prior alone would hold it).  SoftmaxReparamSVI on such a response throws the order away and spends K D parameters,
BLRReparamSVI treats the grades as numbers; this is the model between them, with ONE coefficient vector and K - 1
thresholds.  A larger x . w moves the response UP the scale.

The data enter one update through one linear predictor per (row, draw), exactly as in svi/glm.py; what is new per draw is
parameter-sized.  The pass (include/bayesic_hip.h, bsc_glm_ordinal_data_pass) reads the draws W [S, P] as the finish
wrote them -- weights and theta side by side -- and returns [ell | G] with G [S, P]: the weights' columns and, behind
them, d ell / d theta.  That is ReparamRegressionBase's contract, so step(), sample(), the finish (bsc_glm_update, or
bsc_glm_fullrank_update, at D := P), covariance() and the all-reduce are the base class's, the way SoftmaxReparamSVI uses
them at D := K D.  Offsets and row weights are svi/glm.py's (svi/_obs.py).

The default start m = 0 is ordered with unit gaps: theta_0 = 0 and every log-gap 0, the cutpoints 0, 1, .. K-2.

Labels are int32.  A label outside [0, K) raises ValueError at construction and in set_batch(tensors) (one min/max,
outside step()); raw-pointer batches are the caller's responsibility -- the pass skips such rows and never reads outside
its table for any int32 value.

``covariance="full"``: q(z) = N(mu, L L^T) through bsc_glm_fullrank_update with D := P, svi/glm.py's layout.  That entry
point's envelope applies: P <= 256 and P % 4 == 0 -- with D % 4 == 0 that is K = 5 -- else ValueError.  The cutpoints are
correlated a posteriori with each other and with every coefficient of a feature whose mean is not 0; a diagonal q
reports them too narrow.

Accuracy envelope: log-gaps theta_j (j >= 1) in [-3, 1.5], i.e. gaps between neighbouring cutpoints from 0.05 to 4.5.

Out of scope, by design of this version: full covariance for P % 4 != 0; probit or other links; category-specific
slopes; groups together with cutpoints; recognition by ReparamVI; MiniBatchLoader (it carries a float y).  There is no
one-call (pass + finish) form, so every update is pass -> all-reduce -> finish.  The multi-rank branch is wired like the
other drivers' and has been exercised at world size 1 only.
"""
import numpy as np

from ._obs import ObsBatch, batch_obs
from ._reparam_base import ReparamRegressionBase, check_covariance, check_lam0, check_n_samples
from .softmax import FULL_MAX_PARAMS, _check_labels

MAX_LEVELS = 8            # csrc/bsc_glm_ordinal.hip: the (draw, class) table of one launch
SLAB_FLOATS = 8 * 256 + 8 + 7 * 8


def check_arguments(n_levels, D, prior_precision, n_samples, covariance, lam0=None):
    """The constructor's checks that need no device; returns (K, P)."""
    check_covariance(covariance)
    K = int(n_levels)
    if not 2 <= K <= MAX_LEVELS:
        raise ValueError("n_levels=%d must be in [2, %d]" % (K, MAX_LEVELS))
    if not float(prior_precision) > 0.0:
        raise ValueError("prior_precision must be positive")
    check_n_samples(n_samples)
    P = int(D) + K - 1
    if covariance == "full" and (P > FULL_MAX_PARAMS or P % 4 != 0):
        raise ValueError("covariance='full' needs D + n_levels - 1 <= %d and a multiple of 4 "
                         "(bsc_glm_fullrank_update); got %d + %d - 1 = %d" % (FULL_MAX_PARAMS, D, K, P))
    check_lam0(lam0, P, "w (%d) | theta (%d)" % (D, K - 1), covariance)
    return K, P


def cutpoints(theta):
    """c [.., K - 1] from theta [.., K - 1] (host float64): c_0 = theta_0, c_j = c_{j-1} + e^{theta_j}."""
    theta = np.asarray(theta, np.float64)
    steps = np.concatenate([theta[..., :1], np.exp(theta[..., 1:])], axis=-1)
    return np.cumsum(steps, axis=-1)


class OrdinalReparamSVI(ObsBatch, ReparamRegressionBase):
    link = "ordinal"          # svi/predict.py: family_of.  (No attribute n_classes: that reads as softmax there.)

    def __init__(self, X, y, n_levels, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, ctx=None,
                 group=None, lam0=None, *, offset=None, weights=None, covariance="diag"):
        """``y`` [B] int32 labels in [0, n_levels), in their order.  ``lam0``: [m | rho] over [w (D) | theta (K - 1)]
        (default m = 0 -- the cutpoints 0, 1, .. K-2 -- and every rho = log 0.1).  ``covariance``: "diag" (the mean-field
        guide, default) or "full" (module docstring; ``lam0`` then in the full layout, default the same start with no
        off-diagonal entries).  ``offset`` / ``weights``: float32 [B], as in GLMReparamSVI.  There is no intercept
        column: the cutpoints are the intercepts.  The labels and the weights are checked here (one synchronisation),
        never in step()."""
        import torch
        if len(getattr(X, "shape", ())) != 2 or len(getattr(y, "shape", ())) != 1 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be [B, D] and y [B]")
        K, P = check_arguments(n_levels, X.shape[1], prior_precision, n_samples, covariance, lam0)
        if isinstance(y, torch.Tensor) and y.dtype != torch.int32:
            raise TypeError("y must be int32, got %s" % (y.dtype,))
        _check_labels(y, K)
        from ..device import default_context
        self.covariance_kind = covariance
        self.n_levels = self.K = K
        self.prior_precision = float(prior_precision)
        self.ctx = ctx or default_context()
        self.X = X if isinstance(X, torch.Tensor) else self.ctx.to_device(X, torch.float32)
        self.y = y if isinstance(y, torch.Tensor) else self.ctx.to_device(y, torch.int32)
        if self.X.dtype != torch.float32:
            raise TypeError("X must be float32")
        if self.X.stride(1) != 1:
            raise ValueError("X must be row-major (unit stride along columns)")
        if self.y.numel() > 1 and self.y.stride(0) != 1:
            raise ValueError("y must be contiguous")
        self.B, self.D = int(self.X.shape[0]), int(self.X.shape[1])
        self._Xarg, self._yarg, self._ldx = self.X, self.y, self.X.stride(0)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        self._init_state(P, lam0, n_total, n_samples, seed, lr, group,
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * SLAB_FLOATS * 4)

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None):
        """Point the next update at another device-resident mini-batch of the same width, with its offset and weights:
        torch tensors (the labels are range-checked: one min/max; the weights finite and >= 0), or raw device pointers
        with `rows` (and `ldx`, default D; unchecked).  None drops offset or weights for this batch."""
        import torch
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] != self.D or X.stride(1) != 1 or \
                    not isinstance(y, torch.Tensor) or y.dim() != 1 or y.shape[0] != X.shape[0] or \
                    (y.numel() > 1 and y.stride(0) != 1):
                raise ValueError("batch must be float32 X [rows, %d] row-major and contiguous y [rows]" % self.D)
            if y.dtype != torch.int32:
                raise TypeError("y must be int32, got %s" % (y.dtype,))
            _check_labels(y, self.K)
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
            self.X, self.y = X, y
            self._Xarg, self._yarg, self._ldx, self.B = X, y, X.stride(0), X.shape[0]
        else:
            self._set_raw_batch(X, y, rows, ldx)
        self._set_obs(offset, weights)

    def data_pass(self):
        self.ctx.call("bsc_glm_ordinal_data_pass", self._Xarg, self._ldx, self._yarg, self._oarg, self._varg, self.B,
                      self.D, self.K, self.W, self.P, self.S, self.ell, self.G)

    # -- posterior predictive (one bsc_ordinal_predict_pass over X for all draws) ----------------------------------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """Posterior predictive for the rows of X: a dict of device tensors ``prob`` (float32 [B, K]) and, with y (int32
        labels; a row whose label is outside [0, K) scores 0), ``lpd`` (float32 [B]) and ``lpd_sum`` (float64 [1]).
        ``draws`` = (Z [S, P], None) reuses draws of svi.predict.posterior_draws; otherwise n_samples (at most 64) are
        drawn on Philox stream 2 with ``seed`` (default: the model's).  ``offset``: float32 [B]; a model fitted with one
        refuses to predict without one.  ``weights`` leave every per-row output alone and make ``lpd_sum`` the weighted
        sum_n v_n lpd_n, with ``weight_sum`` = sum_n v_n (float64 [1])."""
        import torch
        from .predict import _check_samples, posterior_draws
        if offset is None and self.has_offset:
            raise ValueError("predict: the model was fitted with an offset; pass offset= for the rows to predict -- a "
                             "silent offset of 0 would shift every row's linear predictor against the cutpoints")
        if draws is None:
            draws = posterior_draws(self, n_samples, seed)
        Z = draws[0]
        S = _check_samples(Z.shape[0])
        if Z.dim() != 2 or Z.shape[1] != self.P or Z.stride(1) != 1 or Z.dtype != torch.float32:
            raise ValueError("draws of the ordinal model are (Z float32 [S, %d], None) as posterior_draws returns "
                             "them" % self.P)
        ctx = self.ctx
        X = X if isinstance(X, torch.Tensor) else ctx.to_device(X, torch.float32)
        if y is not None and not isinstance(y, torch.Tensor):
            y = np.asarray(y)
            if not np.issubdtype(y.dtype, np.integer):
                raise TypeError("y must hold integer class labels (int32), got %s" % (y.dtype,))
            y = ctx.to_device(y, torch.int32)
        if X.dtype != torch.float32:
            raise TypeError("X must be float32")
        if y is not None and y.dtype != torch.int32:
            raise TypeError("y must be int32, got %s" % (y.dtype,))
        if X.dim() != 2 or (y is not None and (y.dim() != 1 or X.shape[0] != y.shape[0])):
            raise ValueError("X must be [B, D] and y [B]")
        if X.stride(1) != 1:
            raise ValueError("X must be row-major (unit stride along columns)")
        if X.shape[1] != self.D:
            raise ValueError("X has %d columns; the model was fitted at D = %d" % (X.shape[1], self.D))
        if y is not None and y.numel() > 1 and y.stride(0) != 1:
            raise ValueError("y must be contiguous")
        B = int(X.shape[0])
        offset, weights = batch_obs(ctx, B, offset, weights)
        ldx = int(X.stride(0)) if B > 1 else max(int(X.stride(0)), self.D)
        ldz = int(Z.stride(0)) if S > 1 else max(int(Z.stride(0)), self.P)
        out = {"prob": torch.empty((B, self.K), dtype=torch.float32, device=ctx.device)}
        if y is not None:
            out["lpd"] = torch.empty(B, dtype=torch.float32, device=ctx.device)
            if weights is None:        # (the weighted sum is formed from the lpd vector below)
                out["lpd_sum"] = torch.zeros(1, dtype=torch.float64, device=ctx.device)
        if B > 0 or y is not None:      # no rows and no score: nothing to write
            ctx.call("bsc_ordinal_predict_pass", X, ldx, y, offset, B, self.D, self.K, Z, ldz, S, out["prob"],
                     out.get("lpd"), out.get("lpd_sum"))
        if weights is not None and y is not None:
            w64 = weights.to(torch.float64)       # a row of weight 0 is dropped by a select, as in the training pass
            out["lpd_sum"] = torch.where(weights > 0, w64 * out["lpd"].to(torch.float64),
                                         torch.zeros_like(w64)).sum().reshape(1)
            out["weight_sum"] = w64.sum().reshape(1)
        return out

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """Mean log predictive density per held-out row (a host float; synchronises); with weights
        sum v lpd / sum v."""
        out = self.predict(X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights)
        if "weight_sum" in out:
            return float(out["lpd_sum"].item()) / float(out["weight_sum"].item())
        return float(out["lpd_sum"].item()) / max(int(out["lpd"].shape[0]), 1)

    # -- host views -----------------------------------------------------------------------------------------------
    def params(self):
        """m and rho (host float64, flat [P]; with a full guide the dense lower-triangular L [P, P] as well), split into
        ``w`` [D] and ``theta`` [K - 1], each as (mean, rho), and ``cutpoints`` [K - 1]: the cutpoints at the guide's
        mean, c_0 = m_theta_0, c_j = c_{j-1} + e^{m_theta_j}."""
        p = self._flat_params()
        D = self.D
        p["w"] = (p["m"][:D], p["rho"][:D])
        p["theta"] = (p["m"][D:], p["rho"][D:])
        p["cutpoints"] = cutpoints(p["m"][D:])
        return p
