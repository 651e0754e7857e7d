"""What the reparameterised regression drivers (svi/glm.py, svi/softmax.py, svi/blr.py) share.

A Gaussian guide over P flattened parameters: ``covariance="diag"`` lam = [m (P) | rho (P)], ``"full"`` lam =
[mu (P) | L packed row-major, lower triangle incl. the diagonal, rho_i = log L_ii in the diagonal slots]
(include/bayesic_hip.h, bsc_glm_fullrank_update).  lam and the draws are double-buffered (index t & 1 is current at the
start of step t + 1) and the noise is drawn NOISE_BLOCK steps ahead by bsc_blr_noise into a ring of two blocks, in its
[S, P + 1] layout (the last column belongs to BLR's scalar latent).

Two classes, not one: ``ReparamDriver`` is what all three drivers share (batch pointers, noise ring, views) and is all
that BLRReparamSVI can take without bending -- it has a scalar latent, sweeps, shards and its own finishes;
``ReparamRegressionBase`` adds the state, first draw, finish and host views of the two drivers whose finish is
bsc_glm_update.  The module-level helpers are pure numpy; torch is imported where a method needs it, so that they can
be used (and tested) without it.
"""
import math

import numpy as np


def full_size(P):
    """Entries of lam in the full layout."""
    return P + P * (P + 1) // 2


def diag_slots(P):
    """Where the full layout keeps rho_i: the diagonal slot of row i of the packed L."""
    i = np.arange(P)
    return P + i * (i + 1) // 2 + i


def unpack_full(lam, P):
    """[mu | packed L] -> (mu [P], dense L [P, P]) with L_ii = e^{rho_i}."""
    rows, cols = np.tril_indices(P)            # row-major lower triangle: the packed order
    L = np.zeros((P, P))
    L[rows, cols] = lam[P:]
    d = np.arange(P)
    L[d, d] = np.exp(L[d, d])
    return np.array(lam[:P], np.float64), L


def rho_of_full(lam, P):
    """rho [P] = log diag L of the full layout."""
    return np.array(np.asarray(lam)[diag_slots(P)])


def default_lam0(P, covariance):
    """The default start (host float64): m = 0, every standard deviation 0.1, no off-diagonal entries."""
    if covariance == "full":
        lam = np.zeros(full_size(P))
        lam[diag_slots(P)] = math.log(0.1)
    else:
        lam = np.zeros(2 * P)
        lam[P:] = math.log(0.1)
    return lam


class ReparamDriver:
    """What all three drivers do alike: the batch pointers, the noise ring and the double-buffer views.  Wants
    self.ctx, .D, .S, .seed, .t, ._lam, ._W and ._noise_dim (the parameter count bsc_blr_noise is called with)."""
    NOISE_BLOCK = 32

    def _float_batch(self, X, y):
        """X [B, D] and y [B] as float32 device tensors (the constructor's checks for a real-valued response)."""
        import torch
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

    def set_batch(self, X, y, rows=None, ldx=None):
        """Point the next update at another device-resident mini-batch of the same width: torch tensors, or raw
        device pointers with `rows` (and `ldx`, default D) -- what MiniBatchLoader.acquire() returns.  The
        mini-batch scaling n_total / batch_rows keeps the batch size the model was built with."""
        import torch
        if isinstance(X, torch.Tensor):
            if X.dtype != torch.float32 or y.dtype != torch.float32 or X.dim() != 2 or \
                    X.shape[1] != self.D or X.stride(1) != 1 or y.shape[0] != X.shape[0]:
                raise ValueError("batch must be float32 X [rows, %d] row-major and y [rows]" % self.D)
            self.X, self.y = X, y
            self._Xarg, self._yarg, self._ldx, self.B = X, y, X.stride(0), X.shape[0]
        else:
            self._set_raw_batch(X, y, rows, ldx)

    def _set_raw_batch(self, X, y, rows, ldx):
        if rows is None:
            raise ValueError("raw device pointers need `rows`")
        self.X = self.y = None
        self._Xarg, self._yarg = int(X), int(y)
        self._ldx, self.B = int(ldx if ldx is not None else self.D), int(rows)

    def _unpack_full(self, lam):
        """unpack_full at this guide's width (self._guide_dim)."""
        return unpack_full(lam, self._guide_dim)

    def _alloc_noise(self, dev):
        import torch
        # noise ring: NOISE_BLOCK steps are drawn per launch, two blocks resident
        self._ring = 2 * self.NOISE_BLOCK
        self._eps = torch.zeros((self._ring, self.S * (self._noise_dim + 1)), dtype=torch.float64, device=dev)
        self._noise_upto = 0   # noise of Philox steps [0, _noise_upto) has been requested

    def _ensure_noise(self, step):
        """Noise of Philox step `step` is in ring row step % ring (drawn a block ahead)."""
        nb = self.NOISE_BLOCK
        while self._noise_upto <= step:
            start = self._noise_upto
            r0 = start % self._ring
            self.ctx.call("bsc_blr_noise", self._noise_dim, self.S, self.seed, start, nb, self._eps[r0:r0 + nb])
            self._noise_upto = start + nb

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


class ReparamRegressionBase(ReparamDriver):
    """Driver state, phases and host views for a model whose P weights have the prior N(0, I / prior_precision) and
    whose data enter through stats = [ell (S) | G (S P)]: the finish is bsc_glm_update / bsc_glm_fullrank_update with
    D := P.  A subclass checks its arguments (lam0's size among them), sets ctx, X, y, B, D, prior_precision and
    covariance_kind, calls _init_state and supplies data_pass() and step()."""

    def _init_state(self, P, n_total, n_samples, seed, lr, group, lam0, slab_bytes):
        """Everything behind the argument checks.  ``slab_bytes`` sizes the pass's workspace once so that step()
        never allocates."""
        import torch
        from .exchange import Exchange
        dev = self.ctx.device
        self.P = self._noise_dim = self._guide_dim = P
        self.S = int(n_samples)
        self.seed = int(seed)
        self.lr = float(lr)
        self.group = group
        self.exchange = Exchange(self.ctx, group)   # RCCL behind the C ABI when ctx has a communicator
        self.world = self.exchange.world
        # global mini-batch rows (all ranks); ranks may hold unequal blocks
        self.batch_rows = self.exchange.global_count(self.B, dev)
        self.n_total = float(n_total) if n_total is not None else self.batch_rows
        S, f64 = self.S, torch.float64
        n_lam = full_size(P) if self.covariance_kind == "full" else 2 * P
        # double-buffered state: index t & 1 is current at the start of step t + 1
        self._lam = torch.zeros((2, n_lam), dtype=f64, device=dev)
        self._lam[0].copy_(torch.as_tensor(default_lam0(P, self.covariance_kind) if lam0 is None else lam0, dtype=f64))
        self._alloc_noise(dev)
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
        self.ctx.reserve(slab_bytes)

    @property
    def scale(self):
        return self.n_total / self.batch_rows

    # -- phases ------------------------------------------------------------------
    def sample(self, step):
        """The first draw w_s = m + e^rho eps_s (every later one comes out of the finish): once per model, in
        float64 on the host from bsc_blr_noise's draws, rounded to float32 as the finish rounds."""
        import torch
        c, P, S = self.cur, self.P, self.S
        self._ensure_noise(step)
        eps = self._eps[step % self._ring].cpu().numpy().reshape(S, P + 1)[:, :P]
        lam = self._lam[c].cpu().numpy()
        if self.covariance_kind == "full":      # w_s = mu + L eps_s
            mu, L = unpack_full(lam, P)
            W = (mu[None, :] + eps @ L.T).astype(np.float32)
        else:
            W = (lam[None, :P] + np.exp(lam[None, P:]) * eps).astype(np.float32)
        self._W[c].copy_(torch.from_numpy(np.ascontiguousarray(W).reshape(-1)))
        self._drawn = True

    def all_reduce(self):
        self.exchange.all_reduce(self.stats)

    def _tail(self, t):
        """The arguments the finishing entry points share; t = Adam step count = Philox step of the NEXT draw."""
        n = 1 - self.cur
        return (self.scale, self.prior_precision, t, self.lr, 0.9, 0.999, 1e-8, self.seed, t,
                self._eps[t % self._ring], 1, self._W[n], self.elbo, self.grad)

    def _finish(self, stats):
        """Gradient + Adam + next draw from all-reduced statistics; flips the double buffer."""
        c = self.cur
        t = self.t + 1
        self._ensure_noise(t)
        name = "bsc_glm_fullrank_update" if self.covariance_kind == "full" else "bsc_glm_update"
        self.ctx.call(name, stats, self._lam[c], self._lam[1 - c], self.m1, self.m2,
                      self._eps[self.t % self._ring], self._W[c], self.P, self.S, *self._tail(t))
        self.t = t

    # -- host views -----------------------------------------------------------
    def _flat_params(self):
        """diag: m, rho.  full: m = mu, the dense lower-triangular L [P, P] and rho = log diag L.  Flat [P]."""
        lam = self.lam.cpu().numpy()
        P = self.P
        if self.covariance_kind == "full":
            m, L = unpack_full(lam, P)
            return dict(m=m, L=L, rho=rho_of_full(lam, P))
        return dict(m=lam[:P], rho=lam[P:])

    def covariance(self):
        """Cov_q over the P flattened weights (P x P, host float64): L L^T of the full guide, diag(e^{2 rho}) of the
        mean-field one."""
        p = self._flat_params()
        if self.covariance_kind == "full":
            return p["L"] @ p["L"].T
        return np.diag(np.exp(2.0 * p["rho"]))
