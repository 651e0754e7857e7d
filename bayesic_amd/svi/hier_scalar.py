"""Random intercepts for the regression families with a learned scalar -- negative binomial, Gamma, Weibull with right
censoring -- by reparameterised-ELBO SVI on the fused pass.

Host-side drivers of csrc/bsc_glm_scalar_group.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  y_n ~ F(l_n, e^tau),   l_n = x_n . w + b[g_n] + o_n          F and its scalar e^tau as in svi/glm_nb.py (the
        dispersion phi), svi/glm_gamma.py (the shape alpha), svi/glm_weibull.py (the shape k; l is the log scale)
        w ~ N(0, I / prior_precision),   b_j | zeta ~ N(0, e^{-zeta}),   e^zeta ~ Gamma(group_a0, group_b0),
        e^tau ~ Gamma(a0, b0)
q:      z = [w (D) | b (J) | zeta | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + J + 2.

The mixed models that grouped data of these kinds call for: overdispersed counts per clinic, store or policy holder,
claim severity per insurer, time to failure per site or batch (a shared-frailty AFT model).  Dropping the groups pools
what the groups explain into the dispersion or the shape; falling back to HierGLMReparamSVI(link="poisson") loses the
dispersion.  The intercept enters through l alone, so the likelihoods are the families' own, and the data enter one
update through stats = [ell | G | H | T] from ONE streaming pass over X (include/bayesic_hip.h,
bsc_glm_scalar_data_pass_groups): H[s, j] = sum_{n : g_n = j} r_ns as in svi/hier_glm.py, T_s = d ell_s / d tau_s as in
the families' drivers.  The group plan is svi/hier_glm.py's -- built when a batch is set, never inside step(): the call
synchronises and is the one place the ids are range-checked.  step() = pass -> all-reduce of stats ->
bsc_glm_scalar_hier_update, ONE finish for the three families (it never sees the likelihood).  lam and the draws (W
[S, D], Bz in the pass's [ceil(S / 8)][J][8] layout, logtau [S]) are double-buffered; the noise comes a block ahead from
bsc_blr_noise with D + J + 1 stream-0 columns (w, b, zeta) and tau's in the last one; the first draw is made on the
host.  The state, the first draw and step() are ReparamDriver's (svi/_reparam_base.py), the plan handling is
GroupPlanBatch's (svi/hier_glm.py), offsets, exposure and row weights svi/glm.py's (svi/_obs.py), and the response is
checked by the family's own check (check_counts, check_positive, pack_response).

predict() / heldout_lpd() (and survival() of the Weibull model) take the rows' ids as ``groups=``, -1 for a group that
was not seen in training, whose intercept is integrated over N(0, e^{-zeta}) under q(zeta) (svi/predict.py;
bsc_scalar_predict_pass_groups).

Accuracy envelopes of tau: the families' (svi/glm_nb.py, svi/glm_gamma.py: [-2.5, 5]; svi/glm_weibull.py: [-2, 4]).

Limits, by design of this version: the guide is mean-field (``covariance="full"`` is refused: P = D + J + 2 is past the
full finish's 256 columns); no interval or left censoring together with groups (``upper=`` is refused: that pass is
not built); no random slopes; ReparamVI does not recognise these log-joints; MiniBatchLoader does not carry ids, offset
and weights.  The multi-rank branch is wired like the other drivers' (every rank builds the plan of its own rows) and
has been exercised at world size 1 only; prediction is single-rank.
"""
import math

import numpy as np

from ._obs import ObsBatch, batch_obs, check_link
from ._reparam_base import ReparamDriver, check_lam0, check_n_samples, check_priors
from .glm_gamma import check_positive
from .glm_nb import check_counts
from .glm_weibull import pack_response
from .hier_glm import MAX_GROUPS, GroupPlanBatch, check_predict_groups

# include/bayesic_hip.h: BSC_SCALAR_*
SCALAR_FAMILIES = {"negbin": 0, "gamma": 1, "weibull": 2}


class HierScalarDriver(GroupPlanBatch, ObsBatch, ReparamDriver):
    """What the three drivers share.  A family states, as class attributes, ``link`` (svi/predict.py's name of the
    family), ``mean_key`` (the key of E_q[e^tau] in params()), ``prior_noun`` (what check_priors calls e^tau) and
    ``has_exposure``, and supplies ``_response(*vectors)``: the checked float32 response the pass reads."""
    workspace_name = "bsc_glm_scalar_group_workspace_bytes"
    has_exposure = True

    @classmethod
    def check_arguments(cls, n_groups, prior_precision, a0, b0, group_a0, group_b0, n_samples, covariance="diag",
                        offset=None, exposure=None):
        """The constructor's checks that need no device."""
        if covariance != "diag":
            raise ValueError("covariance=%r: %s has the mean-field guide only (covariance='diag'); the "
                             "full-covariance finish stops at 256 columns and P = D + J + 2 is past it"
                             % (covariance, cls.__name__))
        if cls.has_exposure:
            check_link("poisson", offset, exposure)      # a log link: exposure is allowed, not together with offset
        if int(n_groups) != n_groups or not 1 <= int(n_groups) <= MAX_GROUPS:
            raise ValueError("n_groups must be an integer in [1, %d], got %r" % (MAX_GROUPS, n_groups))
        check_priors(prior_precision, a0, b0, cls.prior_noun)
        if not (float(group_a0) > 0.0 and float(group_b0) > 0.0):
            raise ValueError("group_a0 and group_b0 (the Gamma prior of the intercepts' precision) must be positive")
        check_n_samples(n_samples)

    def _construct(self, X, response, groups, n_groups, n_total, n_samples, seed, lr, prior_precision, a0, b0, group_a0,
                   group_b0, ctx, group, lam0, offset, weights, exposure, covariance):
        """The constructor; ``response``: the tuple of vectors the family's _response takes."""
        self.check_arguments(n_groups, prior_precision, a0, b0, group_a0, group_b0, n_samples, covariance, offset,
                             exposure)
        y = self._response(*response)                 # a host response: before a device is asked for
        from ..device import default_context
        self._family = SCALAR_FAMILIES[self.link]
        self.covariance_kind = "diag"
        self.J = int(n_groups)
        self.prior_precision, self.a0, self.b0 = float(prior_precision), float(a0), float(b0)
        self.group_a0, self.group_b0 = float(group_a0), float(group_b0)
        self.ctx = ctx or default_context()
        self._float_batch(X, y)
        self._set_obs(*batch_obs(self.ctx, self.B, offset, weights, exposure))
        self.has_offset = self._oarg is not None      # predict() refuses to run without one
        groups = self._checked_groups(groups, self.B)
        D, J, S = self.D, self.J, int(n_samples)
        P = D + J + 2
        check_lam0(lam0, P, "w (%d) | b (%d) | zeta | tau" % (D, J))
        import torch
        # stats = [ell | G | H | T]; the pass's workspace is reserved with the plan (_build_plan)
        self._init_state(P, lam0, n_total, S, seed, lr, group, noise_dim=P - 1, w_cols=D, n_stats=S * (2 + D + J))
        self.H = self.stats[S + S * D:S + S * D + S * J]
        self.T = self.stats[S + S * D + S * J:]
        self._chunks = (S + 7) // 8
        self._Bz = torch.zeros((2, self._chunks * J * 8), dtype=torch.float32, device=self.ctx.device)
        self._logtau = torch.zeros((2, S), dtype=torch.float32, device=self.ctx.device)
        self._set_groups(groups)

    @property
    def Bz(self):
        return self._Bz[self.cur]

    @property
    def logtau(self):
        return self._logtau[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def sample(self, step):
        """The first draw (first_draw) of w, b and tau, rounded to float32 as the finish rounds.  zeta is drawn where it
        is used."""
        import torch
        z = self._first_draw(step).astype(np.float32)
        D, J = self.D, self.J
        self._store_W(z, D)
        self._Bz[self.cur].copy_(torch.from_numpy(self.chunked(z[:, D:D + J])))
        self._logtau[self.cur].copy_(torch.from_numpy(np.ascontiguousarray(z[:, self.P - 1])))
        self._drawn = True

    def data_pass(self):
        self.ctx.call("bsc_glm_scalar_data_pass_groups", self._family, self._Xarg, self._ldx, self._yarg, self._oarg,
                      self._varg, self._garg, self.plan, self.B, self.D, self.J, self.W, self.Bz, self.logtau, self.S,
                      self.ell, self.G, self.H, self.T)

    def _finish(self, stats):
        c, n, t = self.cur, 1 - self.cur, self.t + 1
        self._ensure_noise(t)
        self.ctx.call("bsc_glm_scalar_hier_update", stats, self._lam[c], self._lam[n], self.m1, self.m2,
                      self._eps[self.t % self._ring], self._W[c], self._Bz[c], self._logtau[c], self.D, self.J, self.S,
                      self.scale, self.prior_precision, self.a0, self.b0, self.group_a0, self.group_b0, t, self.lr, 0.9,
                      0.999, 1e-8, self.seed, t, self._eps[t % self._ring], 1, self._W[n], self._Bz[n],
                      self._logtau[n], self.elbo, self.grad)
        self.t = t

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
        """m and rho (host float64) whole and split: w [D], b [J], zeta and tau (scalars), each as (mean, rho), and
        ``mean_key`` = E_q[e^tau] = exp(m_tau + e^{2 rho_tau} / 2)."""
        lam = self.lam.cpu().numpy()
        D, J, P = self.D, self.J, self.P
        m, rho = lam[:P], lam[P:]
        out = dict(m=m, rho=rho, w=(m[:D], rho[:D]), b=(m[D:D + J], rho[D:D + J]), zeta=(m[P - 2], rho[P - 2]),
                   tau=(m[P - 1], rho[P - 1]))
        out[self.mean_key] = math.exp(m[P - 1] + 0.5 * math.exp(2.0 * rho[P - 1]))
        return out


class _CheckedY(HierScalarDriver):
    """The two families whose response is one checked vector y."""

    def __init__(self, X, y, groups, n_groups, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0,
                 a0=1.0, b0=0.1, group_a0=1.0, group_b0=1.0, ctx=None, group=None, lam0=None, *, offset=None,
                 weights=None, exposure=None, covariance="diag"):
        """``groups``: int32 [B], ids in [0, n_groups) (checked here and in set_batch, where the plan is built).
        ``a0``, ``b0``: the Gamma(shape, rate) prior of e^tau, ``group_a0``, ``group_b0``: that of the intercepts'
        precision e^zeta.  ``lam0``: [m | rho] over [w (D) | b (J) | zeta | tau].  The rest as in the family's driver
        without groups."""
        self._construct(X, (y,), groups, n_groups, n_total, n_samples, seed, lr, prior_precision, a0, b0, group_a0,
                        group_b0, ctx, group, lam0, offset, weights, exposure, covariance)

    def _response(self, y):
        self.check_response(y)
        return y

    def set_batch(self, X, y, rows=None, ldx=None, offset=None, weights=None, groups=None, plan=None):
        """GroupPlanBatch.set_batch with y checked as in the constructor (tensors; raw pointers are taken as they
        are)."""
        import torch
        if isinstance(X, torch.Tensor) and groups is not None:
            self.check_response(y)
        super().set_batch(X, y, rows=rows, ldx=ldx, offset=offset, weights=weights, groups=groups, plan=plan)


class HierNegBinReparamSVI(_CheckedY):
    """Negative-binomial regression with random intercepts: NegBinReparamSVI's likelihood and dispersion phi = e^tau
    (``a0``, ``b0``), HierGLMReparamSVI's groups (``group_a0``, ``group_b0``); params() reports phi_mean."""
    link = "negbin"
    mean_key, prior_noun = "phi_mean", "the dispersion"
    check_response = staticmethod(check_counts)


class HierGammaReparamSVI(_CheckedY):
    """Gamma regression (log link) with random intercepts: GammaReparamSVI's likelihood and shape alpha = e^tau;
    params() reports shape_mean."""
    link = "gamma"
    mean_key, prior_noun = "shape_mean", "the shape"
    check_response = staticmethod(check_positive)


UPPER_MSG = ("upper= (interval and left censoring) together with groups is not built: the grouped pass has the "
             "right-censored Weibull link only; WeibullReparamSVI takes upper= without groups")


class HierWeibullReparamSVI(HierScalarDriver):
    """Weibull AFT regression with right censoring and random intercepts (a shared log-normal frailty on the scale):
    WeibullReparamSVI's likelihood, signed response and shape k = e^tau; params() reports shape_mean."""
    link = "weibull"
    mean_key, prior_noun = "shape_mean", "the shape"
    has_exposure = False

    def __init__(self, X, time, groups, n_groups, event=None, n_total=None, n_samples=8, seed=1234, lr=1e-2,
                 prior_precision=1.0, a0=1.0, b0=0.1, group_a0=1.0, group_b0=1.0, ctx=None, group=None, lam0=None, *,
                 upper=None, offset=None, weights=None, covariance="diag"):
        """``time`` [B] finite and > 0; ``event`` [B] bool or 0/1, None = every row an event; ``groups``: int32 [B], ids
        in [0, n_groups).  ``upper`` is refused (module docstring).  The rest as in HierNegBinReparamSVI."""
        if upper is not None:
            raise NotImplementedError(UPPER_MSG)
        self._construct(X, (time, event), groups, n_groups, n_total, n_samples, seed, lr, prior_precision, a0, b0,
                        group_a0, group_b0, ctx, group, lam0, offset, weights, None, covariance)

    def _response(self, time, event=None):
        return pack_response(time, event)

    def set_batch(self, X, time, event=None, rows=None, ldx=None, offset=None, weights=None, groups=None, plan=None,
                  *, upper=None):
        """GroupPlanBatch.set_batch with the batch's censoring flags: tensors (time and event checked as in the
        constructor) with tensor X; with raw device pointers ``time`` is the signed vector and ``event`` not allowed."""
        import torch
        if upper is not None:
            raise NotImplementedError(UPPER_MSG)
        if isinstance(X, torch.Tensor):
            if groups is not None:
                time = pack_response(time, event)
        elif event is not None:
            raise ValueError("with raw device pointers pass the signed vector where(event, time, -time) as time; "
                             "event= is for tensors")
        super().set_batch(X, time, rows=rows, ldx=ldx, offset=offset, weights=weights, groups=groups, plan=plan)

    def _signed(self, time, event):
        if time is None:
            if event is not None:
                raise ValueError("event= needs time=")
            return None
        return pack_response(time, event)

    def predict(self, X, time=None, event=None, groups=None, n_samples=64, seed=None, draws=None, offset=None,
                weights=None):
        """``mean`` = E t and ``var`` = Var t per row and, with ``time``, ``lpd`` and ``lpd_sum``: the log predictive
        density at an event, the log predictive SURVIVAL probability at a censored time.  ``groups`` as in
        HierNegBinReparamSVI.predict."""
        return super().predict(X, self._signed(time, event), groups=groups, n_samples=n_samples, seed=seed, draws=draws,
                               offset=offset, weights=weights)

    def heldout_lpd(self, X, time, event=None, groups=None, n_samples=64, seed=None, draws=None, offset=None,
                    weights=None):
        return super().heldout_lpd(X, self._signed(time, event), groups=groups, n_samples=n_samples, seed=seed,
                                   draws=draws, offset=offset, weights=weights)

    def survival(self, X, t, groups=None, n_samples=64, seed=None, draws=None, offset=None):
        """S(t_n | x_n, g_n) = P(T_n > t_n) under the posterior predictive, float32 [B] on the device: one predictive
        pass with every row censored at t_n, exponentiated."""
        import torch
        y = -pack_response(t)                     # t checked like a duration, every row censored
        return torch.exp(super().predict(X, y, groups=groups, n_samples=n_samples, seed=seed, draws=draws,
                                         offset=offset)["lpd"])
