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

Data parallelism is wired as in svi/blr.py: each rank holds a block of mini-batch rows, and the one exchange per
update is an all-reduce(sum) of the float64 vector [ell (S) | G (S*D)] between the pass and the finish.  That branch
(the one every update of the full guide takes) has been exercised at world size 1 only.
"""
import math

import torch

from ..device import default_context
from .exchange import Exchange

# include/bayesic_hip.h: BSC_GLM_*
LINKS = {"logistic": 0, "poisson": 1}


class GLMReparamSVI:
    NOISE_BLOCK = 32

    def __init__(self, X, y, link="logistic", n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0,
                 ctx=None, group=None, lam0=None, covariance="diag"):
        """``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the
        full layout, default: the mean-field default's mu and rho with zero off-diagonal entries)."""
        if covariance not in ("diag", "full"):
            raise ValueError("covariance must be 'diag' or 'full', got %r" % (covariance,))
        self.covariance_kind = covariance
        if link not in LINKS:
            raise ValueError("link must be 'logistic' or 'poisson', got %r" % (link,))
        self.link, self._link = link, LINKS[link]
        self.ctx = ctx or default_context()
        dev = self.ctx.device
        self.X = X if isinstance(X, torch.Tensor) else self.ctx.to_device(X, torch.float32)
        self.y = y if isinstance(y, torch.Tensor) else self.ctx.to_device(y, torch.float32)
        if self.X.dtype != torch.float32 or self.y.dtype != torch.float32:
            raise TypeError("X and y must be float32")
        if self.X.dim() != 2 or self.y.dim() != 1 or self.X.shape[0] != self.y.shape[0]:
            raise ValueError("X must be [B, D] and y [B]")
        if self.X.stride(1) != 1:
            raise ValueError("X must be row-major (unit stride along columns)")
        self.B, self.D = self.X.shape
        self._Xarg, self._yarg, self._ldx = self.X, self.y, self.X.stride(0)
        self.S = int(n_samples)
        self.seed = int(seed)
        self.lr = float(lr)
        self.prior_precision = float(prior_precision)
        if not self.prior_precision > 0.0:
            raise ValueError("prior_precision must be positive")
        self.group = group
        self.exchange = Exchange(self.ctx, group)   # RCCL behind the C ABI when ctx has a communicator
        self.world = self.exchange.world
        # global mini-batch rows (all ranks); ranks may hold unequal blocks
        self.batch_rows = self.exchange.global_count(self.B, dev)
        self.n_total = float(n_total) if n_total is not None else self.batch_rows
        D, S = self.D, self.S
        f64 = torch.float64
        # double-buffered state: index t & 1 is current at the start of step t + 1
        n_lam = D + D * (D + 1) // 2 if covariance == "full" else 2 * D
        self._lam = torch.zeros((2, n_lam), dtype=f64, device=dev)
        if lam0 is None:
            if covariance == "full":
                diag = torch.arange(D, device=dev)
                self._lam[0, D + diag * (diag + 1) // 2 + diag] = math.log(0.1)
            else:
                self._lam[0, D:] = math.log(0.1)
        else:
            lam0 = torch.as_tensor(lam0, dtype=f64)
            if covariance == "full" and lam0.numel() != n_lam:
                raise ValueError("lam0 has %d entries; covariance='full' at D = %d needs %d" % (lam0.numel(), D, n_lam))
            self._lam[0].copy_(lam0)
        # noise ring: NOISE_BLOCK steps are drawn per launch, two blocks resident
        self._ring = 2 * self.NOISE_BLOCK
        self._eps = torch.zeros((self._ring, S * (D + 1)), dtype=f64, device=dev)
        self._noise_upto = 0   # noise of Philox steps [0, _noise_upto) has been requested
        self._W = torch.zeros((2, S * D), dtype=torch.float32, device=dev)
        self.m1 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.m2 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.grad = torch.zeros(n_lam, dtype=f64, device=dev)
        self.elbo = torch.zeros(1, dtype=f64, device=dev)
        self.stats = torch.zeros(S * (D + 1), dtype=f64, device=dev)  # [ell | G]
        self.ell = self.stats[:S]
        self.G = self.stats[S:]
        self.t = 0
        self._drawn = False
        # size the slab once so step() never allocates
        self.ctx.reserve((4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 8) * 4)

    def set_batch(self, X, y, rows=None, ldx=None):
        """Point the next update at another device-resident mini-batch of the same width: torch tensors, or raw
        device pointers with `rows` (and `ldx`, default D) -- what MiniBatchLoader.acquire() returns.  The
        mini-batch scaling n_total / batch_rows keeps the batch size the model was built with."""
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.float32 or y.dtype != torch.float32 or X.dim() != 2 or \
                    X.shape[1] != self.D or X.stride(1) != 1 or y.shape[0] != X.shape[0]:
                raise ValueError("batch must be float32 X [rows, %d] row-major and y [rows]" % self.D)
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
            self.ctx.call("bsc_blr_noise", self.D, self.S, self.seed, start, nb, self._eps[r0:r0 + nb])
            self._noise_upto = start + nb

    # -- phases ------------------------------------------------------------------
    def sample(self, step):
        """The first draw w_s = m + e^rho eps_s (every later one comes out of the finish): once per model, in
        float64 on the host from bsc_blr_noise's draws, rounded to float32 as the finish rounds."""
        import numpy as np
        c, D, S = self.cur, self.D, self.S
        self._ensure_noise(step)
        eps = self._eps[step % self._ring].cpu().numpy().reshape(S, D + 1)[:, :D]
        lam = self._lam[c].cpu().numpy()
        if self.covariance_kind == "full":      # w_s = mu + L eps_s
            mu, L = self._unpack_full(lam)
            W = (mu[None, :] + eps @ L.T).astype(np.float32)
        else:
            W = (lam[None, :D] + np.exp(lam[None, D:]) * eps).astype(np.float32)
        self._W[c].copy_(torch.from_numpy(np.ascontiguousarray(W).reshape(-1)))
        self._drawn = True

    def _unpack_full(self, lam):
        """[mu | packed L] -> (mu [D], dense L [D, D]) with L_ii = e^{rho_i}."""
        import numpy as np
        D = self.D
        rows, cols = np.tril_indices(D)            # row-major lower triangle: the packed order
        L = np.zeros((D, D))
        L[rows, cols] = lam[D:]
        d = np.arange(D)
        L[d, d] = np.exp(L[d, d])
        return np.array(lam[:D], np.float64), L

    def data_pass(self):
        self.ctx.call("bsc_glm_data_pass", self._link, self._Xarg, self._ldx, self._yarg, self.B, self.D, self.W,
                      self.S, self.ell, self.G)

    def all_reduce(self):
        self.exchange.all_reduce(self.stats)

    def _tail(self, t):
        """The arguments the two finishing entry points share; t = Adam step count = Philox step of the NEXT draw."""
        n = 1 - self.cur
        return (self.scale, self.prior_precision, t, self.lr, 0.9, 0.999, 1e-8, self.seed, t,
                self._eps[t % self._ring], 1, self._W[n], self.elbo, self.grad)

    def _finish(self, stats):
        """Gradient + Adam + next draw from all-reduced statistics; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1
        self._ensure_noise(t)
        name = "bsc_glm_fullrank_update" if self.covariance_kind == "full" else "bsc_glm_update"
        self.ctx.call(name, stats, self._lam[c], self._lam[n], self.m1, self.m2,
                      self._eps[self.t % self._ring], self._W[c], self.D, self.S, *self._tail(t))
        self.t = t

    def _pass_update(self):
        """bsc_glm_pass_update: the pass and the finish in one call; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1
        self._ensure_noise(t)
        self.ctx.call("bsc_glm_pass_update", self._link, self._Xarg, self._ldx, self._yarg, self.B, self.D,
                      self._lam[c], self._lam[n], self.m1, self.m2, self._eps[self.t % self._ring], self._W[c],
                      self.S, *self._tail(t))
        self.t = t

    def step(self):
        """One ELBO-gradient update; asynchronous on the context stream."""
        if not self._drawn:
            self.sample(self.t)  # Philox step index == number of completed updates
        if self.world == 1 and not self.exchange.rccl and self.S <= 8 and self.covariance_kind == "diag":
            self._pass_update()
        else:
            self.data_pass()
            self.all_reduce()
            self._finish(self.stats)

    # -- posterior predictive (svi/predict.py: one bsc_predict_pass over X for all draws) --------
    def predict(self, X, y=None, n_samples=64, seed=None, draws=None):
        from .predict import predict
        return predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws)

    def heldout_lpd(self, X, y, n_samples=64, seed=None, draws=None):
        """Mean log predictive density per held-out row (a host float)."""
        from .predict import heldout_lpd
        return heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws)

    # -- host views -----------------------------------------------------------
    def params(self):
        """diag: m, rho.  full: m = mu [D], the dense lower-triangular L [D, D] and rho = log diag L."""
        import numpy as np
        lam = self.lam.cpu().numpy()
        if self.covariance_kind == "full":
            m, L = self._unpack_full(lam)
            d = np.arange(self.D)
            return dict(m=m, L=L, rho=np.array(lam[self.D + d * (d + 1) // 2 + d]))
        return dict(m=lam[:self.D], rho=lam[self.D:])

    def covariance(self):
        """Cov_q(w) (D x D, host float64): L L^T of the full guide, diag(e^{2 rho}) of the mean-field one."""
        import numpy as np
        if self.covariance_kind == "full":
            _, L = self._unpack_full(self.lam.cpu().numpy())
            return L @ L.T
        return np.diag(np.exp(2.0 * self.params()["rho"]))
