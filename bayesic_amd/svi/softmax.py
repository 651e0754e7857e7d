"""Reparameterised-ELBO SVI for multi-class softmax regression on one fused pass.

Host-side driver of csrc/bsc_softmax.hip; every numeric step is a C-ABI call into libbayesic_hip.so.  The reference
has no inference code -- this is README.md:51 (reparameterisation-trick gradient, refs [10][11][12]) with
mini-batch scaling per README.md:69-79 for the K-class likelihood, the next member of svi/glm.py's family.

Model:  y_n ~ Categorical(softmax(W x_n)),  W in R^{K x D},  every entry ~ N(0, 1 / prior_precision)
q:      vec(W) ~ N(m, diag e^{2 rho});  lam = [m (K D) | rho (K D)], flattened parameter p = k D + d.

All K classes are parameterised (no reference class is pinned): the prior makes the posterior proper.  With
l_nsk = x_n . W_s[k] the data enter one update only through ell_s = sum_n (l_ns,y_n - logsumexp_k l_nsk) and
G_s[k] = sum_n (1[y_n = k] - softmax_k(l_ns)) x_n: bsc_softmax_data_pass streams X once per floor(16 / K) draws, and
the finish is svi/glm.py's -- bsc_glm_update with D := K D on stats = [ell (S) | G (S K D)] (its ELBO and gradient
hold for any model of the form "P Gaussian-prior weights, data through ell and G").  lam and the draws are
double-buffered and the noise is drawn a block ahead by bsc_blr_noise(D := K D) in its [S, K D + 1] layout (Philox
stream 0; the last column is not read), as in svi/glm.py.  There is no one-call slab route: every update is
ReparamDriver's step(), data_pass() -> all_reduce() -> finish.  An intercept is a column of ones in X.

Labels are int32.  A label outside [0, K) raises ValueError at construction and in set_batch(tensors) (one min/max,
outside step()); raw-pointer batches are the caller's responsibility -- the pass skips such rows, it never uses a
label as an address.

``covariance="full"``: q(vec W) = N(mu, L L^T) through bsc_glm_fullrank_update with D := K D, svi/glm.py's layout
lam = [mu (K D) | L packed row-major, lower triangle incl. the diagonal, rho_i in the diagonal slots].  That entry
point's envelope applies: K D <= 256 and K D % 4 == 0, else ValueError.

Data parallelism is wired as in svi/glm.py: each rank holds a block of mini-batch rows and the one exchange per
update is an all-reduce(sum) of the float64 stats vector between the pass and the finish.  That branch has been
exercised at world size 1 only.
"""
import numpy as np
import torch

from ..device import default_context
from ._reparam_base import ReparamRegressionBase, full_size

MAX_CLASSES = 16          # csrc/bsc_softmax.hip: the sixteen (draw, class) columns of one launch
FULL_MAX_PARAMS = 256     # bsc_glm_fullrank_update's envelope
SLAB_FLOATS = 16 * 256 + 8


def _check_labels(y, K, what="y"):
    """Integer labels inside [0, K): one min/max (synchronises when y is on the device)."""
    if isinstance(y, torch.Tensor):
        if y.dtype.is_floating_point or y.dtype == torch.bool:
            raise TypeError("%s must hold integer class labels (int32), got %s" % (what, y.dtype))
        if y.numel():
            lo, hi = int(y.min().item()), int(y.max().item())
        else:
            lo, hi = 0, 0
    else:
        y = np.asarray(y)
        if not np.issubdtype(y.dtype, np.integer):
            raise TypeError("%s must hold integer class labels (int32), got %s" % (what, y.dtype))
        lo, hi = (int(y.min()), int(y.max())) if y.size else (0, 0)
    if lo < 0 or hi >= K:
        raise ValueError("%s has labels in [%d, %d]; n_classes = %d needs them in [0, %d)" % (what, lo, hi, K, K))


class SoftmaxReparamSVI(ReparamRegressionBase):
    link = None               # svi/predict.py: not a GLM link

    def __init__(self, X, y, n_classes, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0,
                 ctx=None, group=None, lam0=None, covariance="diag"):
        """``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the
        full layout, default: the mean-field default's mu and rho with zero off-diagonal entries)."""
        if covariance not in ("diag", "full"):
            raise ValueError("covariance must be 'diag' or 'full', got %r" % (covariance,))
        self.covariance_kind = covariance
        K = int(n_classes)
        if not 2 <= K <= MAX_CLASSES:
            raise ValueError("n_classes=%d must be in [2, %d]" % (K, MAX_CLASSES))
        self.n_classes = self.K = K
        self.prior_precision = float(prior_precision)
        if not self.prior_precision > 0.0:
            raise ValueError("prior_precision must be positive")
        if len(X.shape) != 2 or len(y.shape) != 1 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be [B, D] and y [B]")
        if isinstance(y, torch.Tensor) and y.dtype != torch.int32:
            raise TypeError("y must be int32, got %s" % (y.dtype,))
        _check_labels(y, K)
        D = int(X.shape[1])
        P = K * D
        if covariance == "full" and (P > FULL_MAX_PARAMS or P % 4 != 0):
            raise ValueError("covariance='full' needs n_classes * D <= %d and a multiple of 4 "
                             "(bsc_glm_fullrank_update); got %d * %d = %d" % (FULL_MAX_PARAMS, K, D, P))
        n_lam = full_size(P) if covariance == "full" else 2 * P
        if lam0 is not None and torch.as_tensor(lam0).numel() != n_lam:
            raise ValueError("lam0 has %d entries; covariance=%r at K * D = %d needs %d"
                             % (torch.as_tensor(lam0).numel(), covariance, P, n_lam))
        self.ctx = ctx or default_context()
        self.X = X if isinstance(X, torch.Tensor) else self.ctx.to_device(X, torch.float32)
        self.y = y if isinstance(y, torch.Tensor) else self.ctx.to_device(y, torch.int32)
        if self.X.dtype != torch.float32:
            raise TypeError("X must be float32")
        if self.X.stride(1) != 1:
            raise ValueError("X must be row-major (unit stride along columns)")
        if self.y.numel() > 1 and self.y.stride(0) != 1:
            raise ValueError("y must be contiguous")
        self.B, self.D = int(self.X.shape[0]), D
        self._Xarg, self._yarg, self._ldx = self.X, self.y, self.X.stride(0)
        # the slab is sized for two workgroups per CU at most
        self._init_state(P, lam0, n_total, n_samples, seed, lr, group,
                         reserve_bytes=(2 * self.ctx.info()["cu_count"] + 8) * SLAB_FLOATS * 4)

    def set_batch(self, X, y, rows=None, ldx=None):
        """Point the next update at another device-resident mini-batch of the same width: torch tensors (the labels
        are range-checked: one min/max), or raw device pointers with `rows` (and `ldx`, default D; labels unchecked).
        The mini-batch scaling n_total / batch_rows keeps the batch size the model was built with."""
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.float32 or X.dim() != 2 or X.shape[1] != self.D or X.stride(1) != 1 or \
                    not isinstance(y, torch.Tensor) or y.dim() != 1 or y.shape[0] != X.shape[0] or \
                    (y.numel() > 1 and y.stride(0) != 1):
                raise ValueError("batch must be float32 X [rows, %d] row-major and contiguous y [rows]" % self.D)
            if y.dtype != torch.int32:
                raise TypeError("y must be int32, got %s" % (y.dtype,))
            _check_labels(y, self.K)
            self.X, self.y = X, y
            self._Xarg, self._yarg, self._ldx, self.B = X, y, X.stride(0), X.shape[0]
        else:
            self._set_raw_batch(X, y, rows, ldx)

    def data_pass(self):
        self.ctx.call("bsc_softmax_data_pass", self._Xarg, self._ldx, self._yarg, self.B, self.D, self.K, self.W,
                      self.S, self.ell, self.G)

    # -- posterior predictive (one bsc_softmax_predict_pass over X for all draws) --------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None):
        """Posterior predictive for the rows of X: a dict of device tensors ``prob`` (float32 [B, K]) and, with y
        (int32 labels; a row whose label is outside [0, K) scores 0), ``lpd`` (float32 [B]) and ``lpd_sum``
        (float64 [1]).  ``draws`` = (W [S, K, D], None) reuses draws of svi.predict.posterior_draws; otherwise
        n_samples (at most 64) are drawn on Philox stream 2 with ``seed`` (default: the model's)."""
        from .predict import _check_samples, posterior_draws
        if draws is None:
            draws = posterior_draws(self, n_samples, seed)
        W = draws[0]
        S = _check_samples(W.shape[0])
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
        ldx = int(X.stride(0)) if B > 1 else max(int(X.stride(0)), self.D)
        out = {"prob": torch.empty((B, self.K), dtype=torch.float32, device=ctx.device)}
        if y is not None:
            out["lpd"] = torch.empty(B, dtype=torch.float32, device=ctx.device)
            out["lpd_sum"] = torch.zeros(1, dtype=torch.float64, device=ctx.device)
        if B > 0 or y is not None:      # no rows and no score: nothing to write
            ctx.call("bsc_softmax_predict_pass", X, ldx, y, B, self.D, self.K, W, S, out["prob"], out.get("lpd"),
                     out.get("lpd_sum"))
        return out

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None):
        """Mean log predictive density per held-out row (a host float; synchronises)."""
        out = self.predict(X, y, n_samples=n_samples, seed=seed, draws=draws)
        return float(out["lpd_sum"].item()) / max(int(out["lpd"].shape[0]), 1)

    # -- host views -----------------------------------------------------------
    def params(self):
        """diag: m, rho, each [K, D].  full: m [K, D], the dense lower-triangular L [K D, K D] and rho = log diag L
        [K, D]."""
        p = self._flat_params()
        p["m"], p["rho"] = p["m"].reshape(self.K, self.D), p["rho"].reshape(self.K, self.D)
        return p
