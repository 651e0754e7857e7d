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
data_pass() -> all_reduce() -> finish.  An intercept is a column of ones in X.

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
import math

import numpy as np
import torch

from ..device import default_context
from .exchange import Exchange

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


class SoftmaxReparamSVI:
    NOISE_BLOCK = 32
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
        self.ctx = ctx or default_context()
        dev = self.ctx.device
        self.X = X if isinstance(X, torch.Tensor) else self.ctx.to_device(X, torch.float32)
        self.y = y if isinstance(y, torch.Tensor) else self.ctx.to_device(y, torch.int32)
        if self.X.dtype != torch.float32:
            raise TypeError("X must be float32")
        if self.X.stride(1) != 1:
            raise ValueError("X must be row-major (unit stride along columns)")
        if self.y.numel() > 1 and self.y.stride(0) != 1:
            raise ValueError("y must be contiguous")
        self.B, self.D, self.P = int(self.X.shape[0]), D, P
        self._Xarg, self._yarg, self._ldx = self.X, self.y, self.X.stride(0)
        self.S = int(n_samples)
        self.seed = int(seed)
        self.lr = float(lr)
        self.group = group
        self.exchange = Exchange(self.ctx, group)   # RCCL behind the C ABI when ctx has a communicator
        self.world = self.exchange.world
        # global mini-batch rows (all ranks); ranks may hold unequal blocks
        self.batch_rows = self.exchange.global_count(self.B, dev)
        self.n_total = float(n_total) if n_total is not None else self.batch_rows
        S = self.S
        f64 = torch.float64
        # double-buffered state: index t & 1 is current at the start of step t + 1
        n_lam = P + P * (P + 1) // 2 if covariance == "full" else 2 * P
        self._lam = torch.zeros((2, n_lam), dtype=f64, device=dev)
        if lam0 is None:
            if covariance == "full":
                diag = torch.arange(P, device=dev)
                self._lam[0, P + diag * (diag + 1) // 2 + diag] = math.log(0.1)
            else:
                self._lam[0, P:] = math.log(0.1)
        else:
            lam0 = torch.as_tensor(lam0, dtype=f64)
            if lam0.numel() != n_lam:
                raise ValueError("lam0 has %d entries; covariance=%r at K * D = %d needs %d"
                                 % (lam0.numel(), covariance, P, n_lam))
            self._lam[0].copy_(lam0)
        # noise ring: NOISE_BLOCK steps are drawn per launch, two blocks resident
        self._ring = 2 * self.NOISE_BLOCK
        self._eps = torch.zeros((self._ring, S * (P + 1)), dtype=f64, device=dev)
        self._noise_upto = 0   # noise of Philox steps [0, _noise_upto) has been requested
        self._W = torch.zeros((2, S * P), dtype=torch.float32, device=dev)
        self.m1 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.m2 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.grad = torch.zeros(n_lam, dtype=f64, device=dev)
        self.elbo = torch.zeros(1, dtype=f64, device=dev)
        self.stats = torch.zeros(S * (P + 1), dtype=f64, device=dev)  # [ell | G]
        self.ell = self.stats[:S]
        self.G = self.stats[S:]
        self.t = 0
        self._drawn = False
        # size the slab once so step() never allocates: two workgroups per CU at most
        self.ctx.reserve((2 * self.ctx.info()["cu_count"] + 8) * SLAB_FLOATS * 4)

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
            if rows is None:
                raise ValueError("raw device pointers need `rows`")
            self.X = self.y = None
            self._Xarg, self._yarg = int(X), int(y)
            self._ldx, self.B = int(ldx if ldx is not None else self.D), int(rows)

    # -- current views ---------------------------------------------------------
    @property
    def cur(self):
        return self.t & 1

    @property
    def lam(self):
        return self._lam[self.cur]

    @property
    def W(self):
        return self._W[self.cur]

    @property
    def eps(self):
        return self._eps[self.t % self._ring]

    @property
    def scale(self):
        return self.n_total / self.batch_rows

    def _ensure_noise(self, step):
        """Noise of Philox step `step` is in ring row step % ring (drawn a block ahead)."""
        nb = self.NOISE_BLOCK
        while self._noise_upto <= step:
            start = self._noise_upto
            r0 = start % self._ring
            self.ctx.call("bsc_blr_noise", self.P, self.S, self.seed, start, nb, self._eps[r0:r0 + nb])
            self._noise_upto = start + nb

    # -- phases ------------------------------------------------------------------
    def sample(self, step):
        """The first draw w_s = m + e^rho eps_s (every later one comes out of the finish): once per model, in
        float64 on the host from bsc_blr_noise's draws, rounded to float32 as the finish rounds."""
        c, P, S = self.cur, self.P, self.S
        self._ensure_noise(step)
        eps = self._eps[step % self._ring].cpu().numpy().reshape(S, P + 1)[:, :P]
        lam = self._lam[c].cpu().numpy()
        if self.covariance_kind == "full":      # w_s = mu + L eps_s
            mu, L = self._unpack_full(lam)
            W = (mu[None, :] + eps @ L.T).astype(np.float32)
        else:
            W = (lam[None, :P] + np.exp(lam[None, P:]) * eps).astype(np.float32)
        self._W[c].copy_(torch.from_numpy(np.ascontiguousarray(W).reshape(-1)))
        self._drawn = True

    def _unpack_full(self, lam):
        """[mu | packed L] -> (mu [K D], dense L [K D, K D]) with L_ii = e^{rho_i}."""
        P = self.P
        rows, cols = np.tril_indices(P)            # row-major lower triangle: the packed order
        L = np.zeros((P, P))
        L[rows, cols] = lam[P:]
        d = np.arange(P)
        L[d, d] = np.exp(L[d, d])
        return np.array(lam[:P], np.float64), L

    def data_pass(self):
        self.ctx.call("bsc_softmax_data_pass", self._Xarg, self._ldx, self._yarg, self.B, self.D, self.K, self.W,
                      self.S, self.ell, self.G)

    def all_reduce(self):
        self.exchange.all_reduce(self.stats)

    def _finish(self, stats):
        """Gradient + Adam + next draw from all-reduced statistics; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1                 # Adam step count = Philox step of the NEXT draw
        self._ensure_noise(t)
        name = "bsc_glm_fullrank_update" if self.covariance_kind == "full" else "bsc_glm_update"
        self.ctx.call(name, stats, self._lam[c], self._lam[n], self.m1, self.m2, self._eps[self.t % self._ring],
                      self._W[c], self.P, self.S, self.scale, self.prior_precision, t, self.lr, 0.9, 0.999, 1e-8,
                      self.seed, t, self._eps[t % self._ring], 1, self._W[n], self.elbo, self.grad)
        self.t = t

    def step(self):
        """One ELBO-gradient update; asynchronous on the context stream."""
        if not self._drawn:
            self.sample(self.t)  # Philox step index == number of completed updates
        self.data_pass()
        self.all_reduce()
        self._finish(self.stats)

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
        K, D, P = self.K, self.D, self.P
        lam = self.lam.cpu().numpy()
        if self.covariance_kind == "full":
            m, L = self._unpack_full(lam)
            d = np.arange(P)
            return dict(m=m.reshape(K, D), L=L, rho=np.array(lam[P + d * (d + 1) // 2 + d]).reshape(K, D))
        return dict(m=lam[:P].reshape(K, D), rho=lam[P:].reshape(K, D))

    def covariance(self):
        """Cov_q(vec W) (K D x K D, host float64): L L^T of the full guide, diag(e^{2 rho}) of the mean-field one."""
        if self.covariance_kind == "full":
            _, L = self._unpack_full(self.lam.cpu().numpy())
            return L @ L.T
        return np.diag(np.exp(2.0 * self.params()["rho"].reshape(-1)))
