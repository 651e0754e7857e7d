"""Reparameterised-ELBO SVI for Bayesian linear regression (BASELINE config 2).

Host-side driver of the device path; every numeric step is a C-ABI call into
libbayesic_hip.so.  The reference has no inference code -- this implements
README.md:51 (reparameterisation-trick gradient, refs [10][11][12]) with
mini-batch scaling per README.md:69-79, on the likelihood decomposition of
bayesic/distribution/base.py:47-69.

Model:  y_n ~ N(x_n.w, s2),  w | s2 ~ N(0, s2 I),  s2 ~ InvGamma(alpha0, beta0)
q:      w ~ N(m, diag e^{2 rho}),  log s2 ~ N(a, e^{2b});  lam = [m, rho, a, b].

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w | xi] (P = D + 1), L lower-triangular with
L_ii = e^{rho_i}; lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal, rho_i in the
diagonal slots] (include/bayesic_hip.h, bsc_blr_fullrank_update).  The data pass is the same; the finish
is bsc_blr_fullrank_update, always behind data_pass() -> all_reduce(), so S > 8, ``reproducible=True``
and the RCCL exchange are the mean-field driver's.  A mean-field guide cannot represent the posterior
correlation of w that correlated features induce and shrinks its marginal variances; the full guide can.

``sweep="alternate"`` (default): the passes over a resident mini-batch alternate their direction
so that each starts in the rows the previous one left in the Infinity Cache (158 instead of 164 us
at 1M x 256; a shard below 256 MiB is read from the cache entirely).  ``sweep="stream"`` always walks
forward with non-temporal loads.

One update is two launches on one GPU -- the streaming data pass and a fused
finish (float64 reduction of the pass partials, ELBO + pathwise gradient, Adam
step, next step's Philox draws) -- with lam and the draws double-buffered.  That state, the noise ring and the
exchange are ReparamDriver's (svi/_reparam_base.py), as for the other reparameterised drivers; the scalar latent xi, the
sweeps, the shards and the finishes are this driver's own.

``reproducible=True``: results are bit-identical on 1, 2, 4 and 8 GPUs.
The global mini-batch is cut into V = 8 virtual shards of equal size; a rank runs one data pass
per shard it holds (the pass's workgroup partition then depends on the shard alone, not on p),
the ranks all-reduce a [V, S(D+1)] float64 buffer in which every row is non-zero on exactly one
rank (adding zeros is exact, so the collective's order does not matter), and every rank adds
the V rows in shard order with one n-ary bsc_elemwise launch.  Off by default: on one GPU it is
eight 125k-row passes instead of one 1M-row pass.

Data parallelism: each rank holds a contiguous block of mini-batch rows.  The
only exchange per update is ONE all-reduce(sum) of the float64 vector
[Q (S), G (S*D)] (16 KB at S=8, D=256) between the pass and the finish; noise is
keyed by (seed, step, sample, parameter) and never by rank, so all ranks apply
the identical update.
"""
import math

import torch

from ..device import default_context
from ._reparam_base import ReparamDriver, full_size, unpack_full

# include/bayesic_hip.h: BSC_SWEEP_*
SWEEP_STREAM, SWEEP_FORWARD_KEEP, SWEEP_BACKWARD_KEEP = 0, 1, 2


class BLRReparamSVI(ReparamDriver):
    VIRTUAL_SHARDS = 8

    def __init__(self, X, y, n_total=None, n_samples=8, seed=1234, lr=1e-2, alpha0=1.0,
                 beta0=1.0, ctx=None, group=None, lam0=None, fused=True, reproducible=False,
                 sweep="alternate", family=None, covariance="diag"):
        """``family`` = (c0, c_xi, s_q, k_w, beta): the log-joint per draw as a member of
        f(w, xi; Q) = c0 + c_xi xi + e^{-xi} (-s_q Q / 2 - k_w |w|^2 / 2 - beta) instead of the
        Normal-InverseGamma model above (bsc_blr_fused_update_general) -- what ``inference.ReparamVI``
        passes when it has recognised such a model in a symbolic log-joint.

        ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the
        full layout, default: the mean-field default's mu and rho with zero off-diagonal entries)."""
        if covariance not in ("diag", "full"):
            raise ValueError("covariance must be 'diag' or 'full', got %r" % (covariance,))
        self.covariance_kind = covariance
        self.family = None if family is None else tuple(float(v) for v in family)
        if self.family is not None and len(self.family) != 5:
            raise ValueError("family must be (c0, c_xi, s_q, k_w, beta)")
        if sweep not in ("alternate", "stream"):
            raise ValueError("sweep must be 'alternate' or 'stream'")
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        D = self.D
        if lam0 is None and covariance == "diag":       # lam = [m | rho | a | b]: every standard deviation 0.1
            lam0 = torch.zeros(2 * D + 2, dtype=torch.float64)
            lam0[D:2 * D] = lam0[2 * D + 1] = math.log(0.1)
        elif lam0 is not None and covariance == "full" and torch.as_tensor(lam0).numel() != full_size(D + 1):
            raise ValueError("lam0 has %d entries; covariance='full' at D = %d needs %d"
                             % (torch.as_tensor(lam0).numel(), D, full_size(D + 1)))
        # z = [w | xi]: W holds w and stats = [Q | G] its statistics; the slab is sized once so step() never allocates
        self._init_state(D + 1, lam0, n_total, n_samples, seed, lr, group, noise_dim=D, w_cols=D,
                         reserve_bytes=(4 * self.ctx.info()["cu_count"] + 8) * (8 * 256 + 8) * 4)
        dev, S = self.ctx.device, self.S
        self.Q = self.ell
        self._xi = torch.zeros((2, S), dtype=torch.float64, device=dev)
        self.alpha0, self.beta0 = float(alpha0), float(beta0)
        self.fused = bool(fused)
        # one call per update (bsc_blr_pass_update: the pass, then the finish from its slab) where the library offers the
        # entry point; a test double without it, or one_launch = False, makes the two calls itself
        self.one_launch = hasattr(getattr(self.ctx, "lib", None), "bsc_blr_pass_update")
        self.reproducible = bool(reproducible)
        # "alternate": successive passes over the SAME resident mini-batch walk it forward, then
        # backward, ..., each leaving the rows it read last in the 256 MiB Infinity Cache for the
        # pass that starts there (include/bayesic_hip.h, bsc_blr_data_pass_sweep).  A batch that
        # has just been swapped in (set_batch) is streamed on its first pass.
        self.sweep = sweep
        self._sweep_next = SWEEP_FORWARD_KEEP
        self._fresh_batch = False
        if self.reproducible:
            V = self.VIRTUAL_SHARDS
            total = int(round(self.batch_rows))
            if total % V != 0:
                raise ValueError("reproducible=True needs the global mini-batch (%d rows) to be a multiple "
                                 "of %d virtual shards" % (total, V))
            self._shard_rows = total // V
            first = self.exchange.row_offset(self.B, dev)
            if first % self._shard_rows != 0 or self.B % self._shard_rows != 0:
                raise ValueError("reproducible=True needs every rank to hold whole virtual shards of %d rows "
                                 "(this rank: rows %d..%d)" % (self._shard_rows, first, first + self.B))
            self._first_shard = first // self._shard_rows
            self._n_shards = self.B // self._shard_rows
            self._vstats = torch.zeros((V, S * (D + 1)), dtype=torch.float64, device=dev)

    def set_batch(self, X, y, rows=None, ldx=None):
        super().set_batch(X, y, rows, ldx)
        self._fresh_batch = True

    def _take_sweep(self):
        """Sweep order of the pass about to be issued (and book-keeping for the one after)."""
        if self.sweep != "alternate" or self.reproducible:
            return SWEEP_STREAM
        if self._fresh_batch:
            # nothing of this batch is cached and it may never be read again: stream it; if it IS
            # read again, that pass walks back from the end
            self._fresh_batch = False
            self._sweep_next = SWEEP_BACKWARD_KEEP
            return SWEEP_STREAM
        code = self._sweep_next
        if self._passes_per_update() & 1:   # an odd number of passes ends at the other side
            self._sweep_next = 3 - code
        return code

    def _passes_per_update(self):
        """Launches of the pass kernel per update, as bsc_blr_data_pass issues them (asked of the library
        once per batch pointer: eight draws per pass, or sixteen while more than eight are left at D = 256)."""
        if self.S <= 8:
            return 1
        key = self._yarg if isinstance(self._yarg, int) else self._yarg.data_ptr()
        if getattr(self, "_pass_count", (None, 0))[0] != key:
            if hasattr(self.ctx, "lib"):
                import ctypes
                n = ctypes.c_int32(0)
                self.ctx.call("bsc_blr_pass_count", self._yarg, self.D, self.S, ctypes.byref(n))
                self._pass_count = (key, int(n.value))
            else:                                   # a test double without the library: eight per pass
                self._pass_count = (key, (self.S + 7) // 8)
        return self._pass_count[1]

    # -- current views (cur, lam, W, eps: ReparamDriver) ----------------------------
    @property
    def xi(self):
        return self._xi[self.cur]

    # -- unfused phases (also the multi-sample-group path) ---------------------
    def sample(self, step):
        c = self.cur
        if self.covariance_kind == "full":
            return self._sample_full(step)
        self._ensure_noise(step)        # (bsc_blr_sample rewrites this row with the same values)
        self.ctx.call("bsc_blr_sample", self._lam[c], self.D, self.S, self.seed, step,
                      self._eps[step % self._ring], self._W[c], self._xi[c])
        self._drawn = True

    def _sample_full(self, step):
        """The first draw (first_draw) of the full guide over z = [w | xi]: w rounded to float32, xi kept float64."""
        import numpy as np
        c, D = self.cur, self.D
        z = self._first_draw(step)
        self._W[c].copy_(torch.from_numpy(np.ascontiguousarray(z[:, :D], np.float32).reshape(-1)))
        self._xi[c].copy_(torch.from_numpy(np.ascontiguousarray(z[:, D])))
        self._drawn = True

    def data_pass(self):
        if self.reproducible:
            return self._data_pass_by_shard()
        self.ctx.call("bsc_blr_data_pass_sweep", self._Xarg, self._ldx, self._yarg, self.B,
                      self.D, self.W, self.S, self.Q, self.G, self._take_sweep())

    def _data_pass_by_shard(self):
        """One pass per virtual shard this rank holds, each into its own row of the [V, n] buffer
        (the other rows stay zero until the all-reduce)."""
        if self.X is None:
            raise ValueError("reproducible=True needs tensor batches (set_batch with raw pointers is not sharded)")
        S, rows = self.S, self._shard_rows
        self.ctx.call("bsc_memset", self._vstats, 0, self._vstats.numel() * 8)
        for k in range(self._n_shards):
            r0 = k * rows
            out = self._vstats[self._first_shard + k]
            self.ctx.call("bsc_blr_data_pass", self.X[r0:r0 + rows], self._ldx, self.y[r0:r0 + rows], rows,
                          self.D, self.W, S, out[:S], out[S:])

    def all_reduce(self):
        if not self.reproducible:
            return super().all_reduce()
        import ctypes
        self.exchange.all_reduce(self._vstats)          # every row is non-zero on one rank only: exact
        V, n = self._vstats.shape
        i64 = lambda v: (ctypes.c_int64 * len(v))(*v)
        ptrs = (ctypes.c_void_p * V)(*[self._vstats[v].data_ptr() for v in range(V)])
        # stats = ((V0 + V1) + V2) + ... in shard order: one n-ary add, the same on every rank count
        self.ctx.call("bsc_elemwise", 0, 1, 1, i64([n]), self.stats, i64([1]), V, ptrs, i64([1] * V))

    def _nig_family(self):
        """Config 2 as a member of the family (bsc_blr_fused_update's coefficients)."""
        scale = self.n_total / self.batch_rows
        half = 0.5 * (scale * self.batch_rows + self.D)
        return (-half * math.log(2.0 * math.pi) + self.alpha0 * math.log(self.beta0) - math.lgamma(self.alpha0),
                -half - self.alpha0, scale, 1.0, self.beta0)

    def _finish(self, stats):
        """Fused gradient + Adam + next draw; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1                  # Adam step count; Philox step of the NEXT draw
        self._ensure_noise(t)
        if self.covariance_kind == "full":
            family = self._nig_family() if self.family is None else self.family
            self.ctx.call("bsc_blr_fullrank_update", stats,
                          self._lam[c], self._lam[n], self.m1, self.m2,
                          self._eps[self.t % self._ring], self._W[c], self._xi[c], self.D, self.S,
                          *family, t, self.lr, 0.9, 0.999, 1e-8, self.seed, t,
                          self._eps[t % self._ring], 1, self._W[n], self._xi[n], self.elbo,
                          self.grad)
        elif self.family is None:
            self.ctx.call("bsc_blr_fused_update", stats,
                          self._lam[c], self._lam[n], self.m1, self.m2,
                          self._eps[self.t % self._ring], self._W[c], self._xi[c], self.D, self.S,
                          self.batch_rows, self.n_total / self.batch_rows, self.alpha0, self.beta0,
                          t, self.lr, 0.9, 0.999, 1e-8, self.seed, t,
                          self._eps[t % self._ring], 1, self._W[n], self._xi[n], self.elbo,
                          self.grad)
        else:
            c0, c_xi, s_q, k_w, beta = self.family
            self.ctx.call("bsc_blr_fused_update_general", stats,
                          self._lam[c], self._lam[n], self.m1, self.m2,
                          self._eps[self.t % self._ring], self._W[c], self._xi[c], self.D, self.S,
                          c0, c_xi, s_q, k_w, beta,
                          t, self.lr, 0.9, 0.999, 1e-8, self.seed, t,
                          self._eps[t % self._ring], 1, self._W[n], self._xi[n], self.elbo,
                          self.grad)
        self.t = t

    def _pass_update(self):
        """bsc_blr_pass_update[_general]: data pass + gradient + Adam + next draw as ONE launch; flips the double buffer."""
        c, n = self.cur, 1 - self.cur
        t = self.t + 1                  # Adam step count; Philox step of the NEXT draw
        self._ensure_noise(t)
        head = (self._Xarg, self._ldx, self._yarg, self.B, self.D, self._take_sweep(),
                self._lam[c], self._lam[n], self.m1, self.m2, self._eps[self.t % self._ring], self._W[c], self._xi[c],
                self.S)
        tail = (t, self.lr, 0.9, 0.999, 1e-8, self.seed, t, self._eps[t % self._ring], 1, self._W[n], self._xi[n],
                self.elbo, self.grad)
        if self.family is None:
            self.ctx.call("bsc_blr_pass_update", *head, self.batch_rows, self.n_total / self.batch_rows, self.alpha0,
                          self.beta0, *tail)
        else:
            self.ctx.call("bsc_blr_pass_update_general", *head, *self.family, *tail)
        self.t = t

    def step(self):
        """One ELBO-gradient update; asynchronous on the context stream."""
        if not self._drawn:
            self.sample(self.t)  # Philox step index == number of completed updates
        if self.fused and self.world == 1 and not self.exchange.rccl and self.S <= 8 and not self.reproducible \
                and self.covariance_kind == "diag":
            if self.one_launch:
                self._pass_update()         # the pass and the finish in one call
            else:
                self.ctx.call("bsc_blr_data_pass_partial_sweep", self._Xarg, self._ldx,
                              self._yarg, self.B, self.D, self.W, self.S, self._take_sweep())
                self._finish(None)
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
        """diag: m, rho, a, b.  full: m = mu [P] and the dense lower-triangular L [P, P] (w first, xi last)."""
        lam = self.lam.cpu().numpy()
        D = self.D
        if self.covariance_kind == "full":
            m, L = unpack_full(lam, D + 1)
            return dict(m=m, L=L)
        return dict(m=lam[:D], rho=lam[D:2 * D], a=lam[2 * D], b=lam[2 * D + 1])

    def covariance(self):
        """Cov_q(z) = L L^T over z = [w | xi] (P x P, host float64) of the full guide; the diagonal
        e^{2 rho}, e^{2 b} of the mean-field one."""
        import numpy as np
        if self.covariance_kind == "full":
            _, L = unpack_full(self.lam.cpu().numpy(), self.D + 1)
            return L @ L.T
        p = self.params()
        return np.diag(np.exp(2.0 * np.concatenate([p["rho"], [p["b"]]])))
