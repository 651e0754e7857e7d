"""What the reparameterised regression drivers (svi/blr.py, svi/glm.py, svi/softmax.py, svi/hier_glm.py, svi/glm_nb.py,
svi/glm_gamma.py, svi/glm_weibull.py) share.

A Gaussian guide over P flattened parameters: ``covariance="diag"`` lam = [m (P) | rho (P)], ``"full"`` lam =
[mu (P) | L packed row-major, lower triangle incl. the diagonal, rho_i = log L_ii in the diagonal slots]
(include/bayesic_hip.h, bsc_glm_fullrank_update; with a scalar latent behind the weights bsc_blr_fullrank_update and
bsc_glm_scalar_fullrank_update).  lam and the draws are double-buffered (index t & 1 is current at the
start of step t + 1) and the noise is drawn NOISE_BLOCK steps ahead by bsc_blr_noise into a ring of two blocks, in its
[S, noise width + 1] layout (the last column belongs to a scalar latent: BLR's xi, the hierarchy's zeta).

``ReparamDriver`` is what all four drivers are built on: the batch pointers and their checks, ONE state set-up
(``_init_state``, told sizes and never who is calling), the noise ring, the host side of the first draw, the exchange
and the default step() = sample once, data_pass -> all_reduce -> _finish.  A driver adds what is its own: BLR its
scalar latent xi, sweeps, shards and finishes; the hierarchy Bz, the group plan and H; softmax its labels.
``ReparamRegressionBase`` adds, for the two drivers whose P weights ARE the draws W and whose finish is bsc_glm_update
(GLM, softmax), that finish and its host views.  ``first_draw`` is the one transform from noise to draws that the
drivers' first step and svi/predict.py's predictive draws both use.  The module-level helpers are pure numpy; torch is
imported where a function needs it, so that they can be used (and tested) without it.
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


def first_draw(lam, eps, P, covariance):
    """Noise eps [S, P] -> draws z [S, P] of the guide lam (host float64): z_s = m + e^rho eps_s of the mean-field
    layout, z_s = mu + L eps_s of the full one.  The drivers' first step (every later draw comes out of a finish) and
    the predictive draws of svi/predict.py; the callers slice, round to float32 and upload."""
    if covariance == "full":
        mu, L = unpack_full(lam, P)
        return mu[None, :] + eps @ L.T
    return lam[None, :P] + np.exp(lam[None, P:]) * eps


def check_priors(prior_precision, a0, b0, gamma_of):
    """prior_precision and the Gamma(a0, b0) prior of ``gamma_of`` (the message's noun)."""
    if not float(prior_precision) > 0.0:
        raise ValueError("prior_precision must be positive")
    if not (float(a0) > 0.0 and float(b0) > 0.0):
        raise ValueError("a0 and b0 (the Gamma prior of %s) must be positive" % gamma_of)


def check_n_samples(n_samples):
    if not 1 <= int(n_samples) <= 64:
        raise ValueError("n_samples must be in [1, 64]")


def check_covariance(covariance):
    if covariance not in ("diag", "full"):
        raise ValueError("covariance must be 'diag' or 'full', got %r" % (covariance,))


def check_lam0(lam0, P, layout, covariance="diag"):
    if lam0 is None:
        return
    if covariance == "full":
        if np.asarray(lam0).size != full_size(P):
            raise ValueError("lam0 has %d entries; covariance='full' ([mu | packed L]) over [%s] needs %d"
                             % (np.asarray(lam0).size, layout, full_size(P)))
    elif np.asarray(lam0).size != 2 * P:
        raise ValueError("lam0 has %d entries; [m | rho] over [%s] needs %d" % (np.asarray(lam0).size, layout, 2 * P))


def scalar_latent_params(lam, D, covariance, mean_key):
    """The host views of a guide over z = [w (D) | tau] whose e^tau is a dispersion or a shape (svi/glm_nb.py,
    svi/glm_gamma.py, svi/glm_weibull.py): m and rho whole and split -- w [D] and tau (scalars), each as (mean, rho) --,
    with ``covariance="full"`` the dense lower-triangular L [P, P] as well, and ``mean_key`` = E_q[e^tau] =
    exp(m_tau + Var_q(tau) / 2).  Var_q(tau) is e^{2 rho_tau} under the mean-field guide and the squared norm of the
    WHOLE last row of L under the full one (tau is correlated with w through that row's off-diagonal entries)."""
    lam = np.asarray(lam, np.float64)
    P = D + 1
    if covariance == "full":
        m, L = unpack_full(lam, P)
        rho = rho_of_full(lam, P)
        out = dict(m=m, L=L, rho=rho)
        var_tau = float((L[D] * L[D]).sum())
    else:
        m, rho = lam[:P], lam[P:]
        out = dict(m=m, rho=rho)
        var_tau = math.exp(2.0 * rho[D])
    out.update(w=(m[:D], rho[:D]), tau=(m[D], rho[D]))
    out[mean_key] = math.exp(m[D] + 0.5 * var_tau)
    return out


def scalar_latent_covariance(lam, D, covariance):
    """Cov_q over z = [w (D) | tau] (P x P, host float64): L L^T of the full guide, diag(e^{2 rho}) of the mean-field
    one."""
    P = D + 1
    if covariance == "full":
        L = unpack_full(np.asarray(lam, np.float64), P)[1]
        return L @ L.T
    return np.diag(np.exp(2.0 * np.asarray(lam, np.float64)[P:]))


def float_batch(ctx, X, y, need_y=True):
    """X [B, D] and y [B] (``need_y=False``: or None) as float32 device tensors: the checks of a real-valued batch."""
    import torch
    X = X if isinstance(X, torch.Tensor) else ctx.to_device(X, torch.float32)
    if need_y or y is not None:
        y = y if isinstance(y, torch.Tensor) else ctx.to_device(y, torch.float32)
    if X.dtype != torch.float32 or (y is not None and y.dtype != torch.float32):
        raise TypeError("X and y must be float32")
    if X.dim() != 2 or (y is not None and (y.dim() != 1 or X.shape[0] != y.shape[0])):
        raise ValueError("X must be [B, D] and y [B]")
    if X.stride(1) != 1:
        raise ValueError("X must be row-major (unit stride along columns)")
    return X, y


class ReparamDriver:
    """What all four drivers do alike.  A subclass checks its arguments, sets ctx, covariance_kind and the batch (X, y,
    B, D, _Xarg, _yarg, _ldx: _float_batch for a real-valued response), calls _init_state and supplies data_pass() and
    _finish(stats); sample() where its draws are more than W, step() where there is a shorter way than the default."""
    NOISE_BLOCK = 32

    def _float_batch(self, X, y):
        self.X, self.y = float_batch(self.ctx, X, y)
        self.B, self.D = self.X.shape
        self._Xarg, self._yarg, self._ldx = self.X, self.y, self.X.stride(0)

    def _init_state(self, P, lam0, n_total, n_samples, seed, lr, group, reserve_bytes=0, noise_dim=None, w_cols=None,
                    n_stats=None):
        """Everything behind the argument checks: the exchange and the mini-batch scale, lam [2, n] of a guide over P
        parameters (n = 2 P, or full_size(P)) started at ``lam0`` (None: default_lam0), the noise ring of
        bsc_blr_noise(noise_dim), the draws W [2, S w_cols] (both widths default to P), the Adam moments, grad, elbo and
        stats = [ell (S) | G (S w_cols)] (``n_stats``: longer than that).  ``reserve_bytes`` sizes the pass's
        workspace once so that step() never allocates."""
        import torch
        from .exchange import Exchange
        dev = self.ctx.device
        self.P, self._noise_dim = P, P if noise_dim is None else noise_dim
        self.S, self.seed, self.lr = int(n_samples), int(seed), float(lr)
        self.group = group
        self.exchange = Exchange(self.ctx, group)   # RCCL behind the C ABI when ctx has a communicator
        self.world = self.exchange.world
        # global mini-batch rows (all ranks); ranks may hold unequal blocks
        self.batch_rows = self.exchange.global_count(self.B, dev)
        self.n_total = float(n_total) if n_total is not None else self.batch_rows
        S, f64 = self.S, torch.float64
        w_cols = P if w_cols is None else w_cols
        n_lam = full_size(P) if self.covariance_kind == "full" else 2 * P
        # double-buffered state: index t & 1 is current at the start of step t + 1
        self._lam = torch.zeros((2, n_lam), dtype=f64, device=dev)
        self._lam[0].copy_(torch.as_tensor(default_lam0(P, self.covariance_kind) if lam0 is None else lam0, dtype=f64))
        self._alloc_noise(dev)
        self._W = torch.zeros((2, S * w_cols), dtype=torch.float32, device=dev)
        self.m1 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.m2 = torch.zeros(n_lam, dtype=f64, device=dev)
        self.grad = torch.zeros(n_lam, dtype=f64, device=dev)
        self.elbo = torch.zeros(1, dtype=f64, device=dev)
        self.stats = torch.zeros(S * (1 + w_cols) if n_stats is None else n_stats, dtype=f64, device=dev)
        self.ell = self.stats[:S]
        self.G = self.stats[S:S + S * w_cols]
        self.t = 0
        self._drawn = False
        if reserve_bytes:
            self.ctx.reserve(reserve_bytes)

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

    @property
    def scale(self):
        return self.n_total / self.batch_rows

    # -- phases ------------------------------------------------------------------
    def _first_draw(self, step):
        """first_draw of the current lam from bsc_blr_noise's draws of `step`: host float64 z [S, P], once per model."""
        self._ensure_noise(step)
        eps = self._eps[step % self._ring].cpu().numpy().reshape(self.S, self._noise_dim + 1)[:, :self.P]
        return first_draw(self._lam[self.cur].cpu().numpy(), eps, self.P, self.covariance_kind)

    def _store_W(self, z, cols):
        """The first ``cols`` columns of a first draw z (float32 [S, P]) into the current W."""
        import torch
        self._W[self.cur].copy_(torch.from_numpy(np.ascontiguousarray(z[:, :cols]).reshape(-1)))

    def _finish_latent(self, name, stats, extra, dims):
        """_finish of a model with a Gamma(a0, b0) prior and one latent besides W, through entry point ``name`` (a
        mean-field finish, or bsc_glm_scalar_fullrank_update, which takes the same arguments); ``extra``: that latent's
        [2, .] double buffer, ``dims``: the sizes the call takes before S."""
        c, n, t = self.cur, 1 - self.cur, self.t + 1
        self._ensure_noise(t)
        self.ctx.call(name, stats, self._lam[c], self._lam[n], self.m1, self.m2, self._eps[self.t % self._ring],
                      self._W[c], extra[c], *dims, self.S, self.scale, self.prior_precision, self.a0, self.b0, t,
                      self.lr, 0.9, 0.999, 1e-8, self.seed, t, self._eps[t % self._ring], 1, self._W[n], extra[n],
                      self.elbo, self.grad)
        self.t = t

    def all_reduce(self):
        self.exchange.all_reduce(self.stats)

    def step(self):
        """One ELBO-gradient update; asynchronous on the context stream."""
        if not self._drawn:
            self.sample(self.t)  # Philox step index == number of completed updates
        self.data_pass()
        self.all_reduce()
        self._finish(self.stats)


class ReparamRegressionBase(ReparamDriver):
    """The finish and the host views of a model whose P weights have the prior N(0, I / prior_precision), are the draws
    W themselves, and meet the data through stats = [ell (S) | G (S P)]: bsc_glm_update / bsc_glm_fullrank_update with
    D := P.  A subclass sets prior_precision besides what ReparamDriver asks."""

    def sample(self, step):
        """The first draw (first_draw), rounded to float32 as the finish rounds."""
        self._store_W(self._first_draw(step).astype(np.float32), self.P)
        self._drawn = True

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
