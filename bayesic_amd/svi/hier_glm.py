"""Random-intercept logistic / Poisson regression by reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_group.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ Bernoulli(sigmoid(l_n))  or  Poisson(exp(l_n)),    l_n = x_n . w + b[g_n] + o_n
        w ~ N(0, I / prior_precision),   b_j | zeta ~ N(0, e^{-zeta}),   tau = e^{zeta} ~ Gamma(a0, b0)
q:      z = [w (D) | b (J) | zeta] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + J + 1.

At prior_precision = 1 and the logistic link this is BASELINE config 5, the model svi/bbvi.py steps with the
score-function estimator at S = 64; the log-prior is ``oracle.svi.bbvi_log_prior``, so the two drivers target the same
posterior.  Here the gradient is pathwise and S = 8 is enough, which keeps the update on ONE streaming pass over X:
besides ell_s and G_s (svi/glm.py) the data enter through H[s, j] = sum_{n : g_n = j} r_ns, the per-group sums of the
row residuals (include/bayesic_hip.h, bsc_glm_data_pass_groups).  That scatter is summed in an order fixed by a GROUP
PLAN (bsc_glm_group_plan) -- built when a batch is set, never inside step(): the call synchronises and is the one
place the ids are range-checked.  step() = pass -> all-reduce of [ell | G | H] -> bsc_glm_hier_update (ELBO, gradient,
Adam, next draws).  lam and the draws (W [S, D] and Bz, the intercepts in the pass's [ceil(S / 8)][J][8] layout) are
double-buffered; the noise comes a block ahead from bsc_blr_noise with D + J stream-0 columns and zeta's in the last
one; the first draw is made on the host.  The state, the first draw and step() are ReparamDriver's
(svi/_reparam_base.py); offsets, exposure and row weights are svi/glm.py's (svi/_obs.py).

predict() / heldout_lpd() (svi/predict.py; csrc/bsc_predict_group.hip, bsc_predict_pass_groups) take the rows' ids as
``groups=``: the predictive needs a per-draw, per-group term in the logit, so a call without them is refused rather
than read as "every row is a new group".  An id of -1 marks a group that was not seen in training: its intercept is
integrated over N(0, e^{-zeta}) under q(zeta).  The ids are range-checked once per call (bsc_group_ids_check).

Limits, by design of this version: the guide is mean-field (``covariance="full"`` is refused: P = D + J + 1 is past the
full finish's 256 columns).  The multi-rank branch is wired like the other drivers' (every rank builds the plan of its
own rows) and has been exercised at world size 1 only; prediction is single-rank.
"""
import ctypes

import numpy as np

from ._obs import LINKS, ObsBatch, batch_obs, check_link
from ._reparam_base import ReparamDriver, check_lam0, check_n_samples, check_priors

MAX_GROUPS = 65536          # include/bayesic_hip.h: BSC_GLM_GROUP_MAX_J


def check_arguments(link, n_groups, prior_precision, a0, b0, covariance, offset, exposure):
    """The constructor's checks that need no device."""
    if covariance != "diag":
        raise ValueError("covariance=%r: HierGLMReparamSVI has the mean-field guide only (covariance='diag'); the "
                         "full-covariance finish stops at 256 columns and P = D + J + 1 is past it" % (covariance,))
    check_link(link, offset, exposure)
    if int(n_groups) != n_groups or not 1 <= int(n_groups) <= MAX_GROUPS:
        raise ValueError("n_groups must be an integer in [1, %d], got %r" % (MAX_GROUPS, n_groups))
    check_priors(prior_precision, a0, b0, "the intercepts' precision")


NO_GROUPS = ("the predictive of a random-intercept model needs a per-draw, per-group term in the logit: pass groups= "
             "(one int32 id per row, -1 for a group not seen in training)")


def check_predict_groups(groups, B):
    """The checks of predict()'s ``groups=`` that need no device: it is there (NotImplementedError otherwise: rows
    without ids are not silently read as new groups), a tensor is int32, a host array holds integers, and either is a
    contiguous [B].  A raw device pointer (an int) is taken as it is."""
    if groups is None:
        raise NotImplementedError(NO_GROUPS)
    if isinstance(groups, (int, np.integer)):
        return
    import torch
    if isinstance(groups, torch.Tensor):
        if groups.dtype != torch.int32:
            raise TypeError("groups must be int32")
        shape, unit = tuple(groups.shape), groups.dim() != 1 or groups.shape[0] <= 1 or groups.stride(0) == 1
    else:
        a = np.asarray(groups)
        if a.dtype.kind not in "iu":
            raise TypeError("groups must hold integers (it is uploaded as int32), got dtype %s" % a.dtype)
        shape, unit = a.shape, True
    if len(shape) != 1 or shape[0] != B or not unit:
        raise ValueError("groups must be a contiguous [%d], one id per row of X" % B)


class GroupPlanBatch:
    """The group ids of a driver's current batch and their plan: what HierGLMReparamSVI and the drivers of
    svi/hier_scalar.py do alike.  The driver has ctx, J, B and _chunks, is an ObsBatch and a ReparamDriver, and names
    the entry point that sizes its pass's workspace."""
    workspace_name = "bsc_glm_group_workspace_bytes"

    def _checked_groups(self, groups, B):
        """The ids of a batch of B rows: a tensor or a host array (checked like y, uploaded as int32), or a raw device
        pointer to B int32 (taken as it is)."""
        import torch
        if groups is None:
            raise ValueError("groups is required: one int32 id in [0, %d) per row" % self.J)
        if isinstance(groups, (int, np.integer)):
            return int(groups)
        g = groups if isinstance(groups, torch.Tensor) else self.ctx.to_device(np.asarray(groups), torch.int32)
        if g.dtype != torch.int32:
            raise TypeError("groups must be int32")
        if g.dim() != 1 or g.shape[0] != B or (B > 1 and g.stride(0) != 1):
            raise ValueError("groups must be a contiguous [%d], one id per row of X" % B)
        return g

    def _build_plan(self, garg, B):
        """(plan, segment count) of B ids.  Synchronises (bsc_glm_group_plan: the ids' range is checked there) and
        reserves the pass's workspace so that step() never allocates."""
        import torch
        lib = self.ctx.lib
        n = int(lib.bsc_glm_group_plan_size(B, self.J))
        if n < 0:
            raise ValueError("a group plan holds at most 2^30 rows and %d groups (B = %d, J = %d)"
                             % (MAX_GROUPS, B, self.J))
        plan = torch.zeros(n, dtype=torch.int32, device=self.ctx.device)
        n_seg = ctypes.c_int32(0)
        self.ctx.call("bsc_glm_group_plan", garg, B, self.J, plan, ctypes.byref(n_seg))
        self.ctx.reserve(int(getattr(lib, self.workspace_name)(self.ctx.handle, B, self.J)))
        return plan, int(n_seg.value)

    def build_plan(self, groups, rows):
        """The group plan of ``rows`` ids, for ``set_batch(..., plan=)``: a loop over a fixed set of batches builds each
        batch's plan once, outside the loop (this call synchronises and range-checks the ids), and set_batch then takes
        it without rebuilding.  ``groups`` as in set_batch.  The pair belongs to these ids, this row count and this
        model's n_groups: the pass does not read a plan whose header names another batch (H comes back NaN)."""
        return self._build_plan(self._checked_groups(groups, int(rows)), int(rows))

    def _set_groups(self, garg, built=None):
        import torch
        self.plan, self.n_segments = built if built is not None else self._build_plan(garg, self.B)
        self.groups = garg if isinstance(garg, torch.Tensor) else None
        self._garg = garg

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None, groups=None, plan=None):
        """ReparamDriver.set_batch with the batch's group ids (required: the plan is rebuilt here, one
        synchronisation) and its offset and weights as in GLMReparamSVI.set_batch.  ``plan``: what build_plan returned
        for these ids; the plan is then not rebuilt (with raw device pointers the call does not synchronise)."""
        import torch
        if groups is None:
            raise ValueError("set_batch needs groups=: the ids of the new rows (the group plan is rebuilt)")
        if isinstance(X, torch.Tensor):
            B = int(X.shape[0])
            offset, weights = batch_obs(self.ctx, B, offset, weights)
        elif rows is None:
            raise ValueError("raw device pointers need `rows`")
        else:
            B = int(rows)
        garg = self._checked_groups(groups, B)
        # (a plan built here refuses bad ids before anything of the driver changes)
        built = plan if plan is not None else self._build_plan(garg, B)
        super().set_batch(X, y, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)
        self._set_groups(garg, built)

    def chunked(self, b):
        """b [S, J] (host) -> the pass's float32 [ceil(S / 8)][J][8] layout, unused slots zero, flat."""
        S, J = b.shape
        out = np.zeros((self._chunks, J, 8), np.float32)
        for s in range(S):
            out[s // 8, :, s % 8] = b[s]
        return out.reshape(-1)


class HierGLMReparamSVI(GroupPlanBatch, ObsBatch, ReparamDriver):
    def __init__(self, X, y, groups, n_groups, link="logistic", n_total=None, n_samples=8, seed=1234, lr=1e-2,
                 prior_precision=1.0, a0=1.0, b0=1.0, offset=None, weights=None, exposure=None, ctx=None, group=None,
                 lam0=None, covariance="diag"):
        """``groups``: int32 [B], ids in [0, n_groups) (checked here and in set_batch, where the plan is built).
        ``group``: the torch.distributed process group of a data-parallel job, as in the other drivers."""
        check_arguments(link, n_groups, prior_precision, a0, b0, covariance, offset, exposure)
        check_n_samples(n_samples)
        from ..device import default_context
        self.link, self._link = link, LINKS[link]
        self.covariance_kind = "diag"
        self.J = int(n_groups)
        self.prior_precision, self.a0, self.b0 = float(prior_precision), float(a0), float(b0)
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        groups = self._checked_groups(groups, self.B)
        D, J, S = self.D, self.J, int(n_samples)
        P = D + J + 1
        check_lam0(lam0, P, "w (%d) | b (%d) | zeta" % (D, J))
        import torch
        # stats = [ell | G | H]; the pass's workspace is reserved with the plan (_build_plan)
        self._init_state(P, lam0, n_total, S, seed, lr, group, noise_dim=D + J, w_cols=D, n_stats=S * (1 + D + J))
        self.H = self.stats[S + S * D:]
        self._chunks = (S + 7) // 8
        self._Bz = torch.zeros((2, self._chunks * J * 8), dtype=torch.float32, device=self.ctx.device)
        self._set_groups(groups)

    @property
    def Bz(self):
        return self._Bz[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def sample(self, step):
        """The first draw (first_draw) of w and b, rounded to float32 as the finish rounds.  zeta is drawn where it is
        used."""
        import torch
        z = self._first_draw(step).astype(np.float32)
        self._store_W(z, self.D)
        self._Bz[self.cur].copy_(torch.from_numpy(self.chunked(z[:, self.D:self.D + self.J])))
        self._drawn = True

    def data_pass(self):
        self.ctx.call("bsc_glm_data_pass_groups", self._link, self._Xarg, self._ldx, self._yarg, self._oarg, self._varg,
                      self._garg, self.plan, self.B, self.D, self.J, self.W, self.Bz, self.S, self.ell, self.G, self.H)

    def _finish(self, stats):
        self._finish_latent("bsc_glm_hier_update", stats, self._Bz, (self.D, self.J))

    # -- the predictive --------------------------------------------------------------------------------------------
    def predict(self, X, y=None, groups=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None,
                weights=None):
        """svi/predict.py's predict with the rows' ids (required; -1 = a group not seen in training)."""
        check_predict_groups(groups, int(X.shape[0]))
        from . import predict as P
        return P.predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                         weights=weights, groups=groups)

    def heldout_lpd(self, X, y, groups=None, n_samples=64, seed=None, draws=None, offset=None, exposure=None,
                    weights=None):
        """svi/predict.py's heldout_lpd with the rows' ids (required, as in predict)."""
        check_predict_groups(groups, int(X.shape[0]))
        from . import predict as P
        return P.heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, exposure=exposure,
                             weights=weights, groups=groups)

    # -- host views -----------------------------------------------------------------------------------------------
    def params(self):
        """m and rho (host float64) whole and split: w [D], b [J], zeta (scalars), each as (mean, rho)."""
        lam = self.lam.cpu().numpy()
        D, J, P = self.D, self.J, self.P
        m, rho = lam[:P], lam[P:]
        return dict(m=m, rho=rho, w=(m[:D], rho[:D]), b=(m[D:D + J], rho[D:D + J]), zeta=(m[P - 1], rho[P - 1]))
