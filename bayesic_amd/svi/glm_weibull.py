"""Weibull survival regression (accelerated failure time) with right censoring and a learned shape by
reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_weibull.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  t_n ~ Weibull(shape k, scale e^{l_n}),   l_n = x_n . w + o_n,   w ~ N(0, I / prior_precision),
        k = e^tau ~ Gamma(a0, b0);   delta_n = 1: the event was seen at t_n,  delta_n = 0: right-censored, the event is
        later than t_n.
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The model for a duration that is only partly observed (time to failure, length of stay, time to churn): the rows that
are still running when the data are cut enter through their survival probability, log S(t) = -e^z, the others through
the density, log f(t) = tau + z - log t - e^z, with z = k (log t - l).  Dropping the censored rows, or treating the
cut-off as the failure time (what a GammaReparamSVI fit of the same data has to do), biases the scale and the shape.
l is the log SCALE, not the log mean: E t = e^l Gamma(1 + 1/k), Var t = e^{2l} (Gamma(1 + 2/k) - Gamma(1 + 1/k)^2).
At k = 1 with every row an event this is the Gamma model at alpha = 1, the exponential distribution.

The censoring flag costs nothing on the device: the driver keeps ONE float32 vector y = where(event, time, -time) --
y_n > 0 is an event at y_n, y_n < 0 is censored at -y_n; a duration is positive, so the sign is free -- and that vector is
what the pass reads (include/bayesic_hip.h, bsc_glm_weibull_data_pass).  With raw device pointers the caller passes the
signed vector.  The data enter one update through ell_s, G_s (svi/glm.py) and T_s = d ell_s / d tau_s, all from ONE
streaming pass over X; the shape draw tau_s rides with the weight draw w_s exactly as NegBinReparamSVI's dispersion and
GammaReparamSVI's shape do, and the finish is theirs (the prior on e^tau has the same form).  step() = pass ->
all-reduce of [ell | G | T] -> bsc_glm_weibull_update; the state, the first draw and step() are ReparamDriver's
(svi/_reparam_base.py), offsets and row weights svi/glm.py's (svi/_obs.py).  There is no ``exposure``: a multiplier on
the scale has no established meaning here, and ``offset`` covers it.

``time`` must be finite and strictly positive, ``event`` a bool or 0/1 array of length B (None: every row is an event).
Both are checked where a batch is set -- the constructor and set_batch, on the host before a device is asked for when
they are host arrays -- and never in step(); raw device pointers are taken as they are.  The pass does not clamp: it is
finite while z = k (log t - l) stays below about 88.

Accuracy envelope: tau in [-2, 4] (k from 0.14 to 55); below it the predictive moments leave float32 (Gamma(1 + 2/k)
overflows near k = 0.06).

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more).  With censoring the shape is correlated a
posteriori with the intercept and with every coefficient that moves the scale; a diagonal q reports it too narrow, and
that width is what predict, heldout_lpd and survival carry on.

Interval and left censoring (``upper=``, keyword-only, on the constructor, set_batch, predict and heldout_lpd): a
float [B] vector of upper ends next to ``time``.  ``inf`` says the row has no upper end and is whatever ``event`` says;
a finite value greater than ``time`` says the event lies in (time, upper] -- found failed at an inspection, known to
the day -- and a finite value on a row with ``time == 0`` says it had already happened when the row was first looked at
(left-censored at ``upper``; only such a row may have ``time == 0``).  With ``event=None`` a row with a finite upper end
is censored and every other row is an event.  Such a row enters through its probability, log(S(a) - S(b)) =
-E_a + log(-expm1(-Delta)) with Delta = E_a expm1(k d) (include/bayesic_hip.h, bsc_glm_weibull_data_pass_interval, has
the forms, the derivatives and the overflow rule: an upper end so far out that the row's upper survival is 0 in float32,
``upper=1e30`` say, is read as absent).  Taking the midpoint or the upper end as the event time biases the shape,
calling the row right-censored at ``time`` throws the upper end away.  On the device it is ONE more float32 vector
(``pack_censored``): 0 = the row is what y says, > 0 = the interval's upper end (y = -time), < 0 = left-censored at its
magnitude (y holds the same value).  The pass with it is the new entry point, and only when an ``upper`` is set: with
``upper=None`` every check, message, call and bit is what it was.  The finishes see [ell | G | T] alone, so
``covariance="full"`` needs nothing new; ``survival`` is unchanged.  With raw device pointers ``upper`` is a raw pointer to
the device encoding.

Random intercepts per group together with the shape (a shared frailty; right censoring only): HierWeibullReparamSVI
(svi/hier_scalar.py).

Out of scope, by design of this version: left truncation (delayed entry);
recognition by ReparamVI (it does not recognise a Weibull log-joint); MiniBatchLoader
(it does not carry offset and weights).  There is no one-call (pass +
finish) form, so every update is pass -> all-reduce -> finish.  The multi-rank branch is wired like the other drivers'
and has been exercised at world size 1 only.
"""
import numpy as np

from ._obs import batch_obs, obs_vector
from ._reparam_base import ReparamDriver
from ._scalar_latent import ScalarLatentDriver

TIME_MSG = "time must be finite and > 0 (a duration; censoring is given by event=, not by a sign)"
EVENT_MSG = "event must be a bool or 0/1 array of length %d, one entry per row (None: every row is an event)"
UPPER_SHAPE_MSG = "upper must be a float array of length %d, one entry per row (inf: no upper end)"
UPPER_NAN_MSG = "upper must not be NaN (inf says that a row has no upper end)"
UPPER_NEG_MSG = "upper must not be negative: it is the upper end of a censoring interval (the device encoding's sign " \
                "is pack_censored's to set)"
UPPER_EVENT_MSG = "an event row (event = 1) cannot have a finite upper: an event seen at time has no interval; pass " \
                  "event = 0 or upper = inf there"
UPPER_INTERVAL_MSG = "an interval-censored row needs upper > time (as float32): the event lies in (time, upper]"
UPPER_LEFT_MSG = "a left-censored row (time == 0) needs a finite upper > 0"
TIME_UPPER_MSG = TIME_MSG + "; only a left-censored row (a finite upper) may have time == 0"


def pack_response(time, event=None):
    """The signed float32 response the pass reads, where(event, time, -time), after the checks of ``time`` (finite and
    > 0 as float32) and ``event`` (bool or 0/1, length B).  Host arrays give a host array; a tensor ``time`` gives a
    tensor on its device (one synchronisation, so it sits outside step())."""
    import torch
    if isinstance(time, torch.Tensor):
        if time.dim() != 1 or not bool((torch.isfinite(time) & (time > 0)).all()):
            raise ValueError(TIME_MSG)
        if event is None:
            return time
        ev = event if isinstance(event, torch.Tensor) else torch.as_tensor(np.asarray(event))
        if ev.dim() != 1 or ev.shape[0] != time.shape[0]:
            raise ValueError(EVENT_MSG % time.shape[0])
        if ev.dtype != torch.bool:
            if not bool(((ev == 0) | (ev == 1)).all()):
                raise ValueError(EVENT_MSG % time.shape[0])
            ev = ev != 0
        return torch.where(ev.to(time.device), time, -time)
    with np.errstate(over="ignore"):
        t = np.asarray(time, np.float32)
    if t.ndim != 1 or not (np.isfinite(t).all() and (t > 0).all()):
        raise ValueError(TIME_MSG)
    if event is None:
        return t
    if isinstance(event, torch.Tensor):
        event = event.cpu().numpy()
    ev = np.asarray(event)
    if ev.ndim != 1 or ev.shape[0] != t.shape[0]:
        raise ValueError(EVENT_MSG % t.shape[0])
    if ev.dtype != np.bool_:
        if ev.dtype.kind not in "iuf" or not ((ev == 0) | (ev == 1)).all():
            raise ValueError(EVENT_MSG % t.shape[0])
        ev = ev != 0
    return np.where(ev, t, -t).astype(np.float32)


def _event_mask(event, B, xp, like):
    """``event`` as a bool mask of length B in ``xp`` (numpy or torch; on ``like``'s device), with pack_response's checks."""
    import torch
    if xp is np:
        if isinstance(event, torch.Tensor):
            event = event.cpu().numpy()
        ev = np.asarray(event)
        if ev.ndim != 1 or ev.shape[0] != B:
            raise ValueError(EVENT_MSG % B)
        if ev.dtype != np.bool_:
            if ev.dtype.kind not in "iuf" or not ((ev == 0) | (ev == 1)).all():
                raise ValueError(EVENT_MSG % B)
            ev = ev != 0
        return ev
    ev = event if isinstance(event, torch.Tensor) else torch.as_tensor(np.asarray(event))
    if ev.dim() != 1 or ev.shape[0] != B:
        raise ValueError(EVENT_MSG % B)
    if ev.dtype != torch.bool:
        if not bool(((ev == 0) | (ev == 1)).all()):
            raise ValueError(EVENT_MSG % B)
        ev = ev != 0
    return ev.to(like.device)


def pack_censored(time, event=None, upper=None):
    """The pair (y, upper) in the device encoding of bsc_glm_weibull_data_pass_interval, after the checks of the module
    docstring (each refusal names the row kind): y = where(event, time, -time) and upper = 0 on a row without an upper
    end; y = -time and upper = the upper end on an interval row; y = upper = -(the upper end) on a left-censored row.
    Host arrays give host arrays, a tensor ``time`` gives tensors on its device (one synchronisation).  ``upper=None``:
    (pack_response(time, event), None)."""
    if upper is None:
        return pack_response(time, event), None
    import torch
    if isinstance(time, torch.Tensor):
        xp, t = torch, time
        u = upper if isinstance(upper, torch.Tensor) else torch.as_tensor(np.asarray(upper))
        if t.dim() != 1:
            raise ValueError(TIME_UPPER_MSG)
        if u.dim() != 1 or u.shape[0] != t.shape[0] or not u.dtype.is_floating_point:
            raise ValueError(UPPER_SHAPE_MSG % t.shape[0])
        if not t.dtype.is_floating_point:
            raise ValueError(TIME_UPPER_MSG)
        t = t.to(torch.float32)                   # the comparisons below are made on what the device reads
        u = u.to(device=t.device, dtype=torch.float32)
    else:
        xp = np
        if isinstance(upper, torch.Tensor):
            upper = upper.cpu().numpy()
        with np.errstate(over="ignore"):
            t = np.asarray(time, np.float32)
            if t.ndim != 1:
                raise ValueError(TIME_UPPER_MSG)
            u = np.asarray(upper)
            if u.ndim != 1 or u.shape[0] != t.shape[0] or u.dtype.kind != "f":
                raise ValueError(UPPER_SHAPE_MSG % t.shape[0])
            u = u.astype(np.float32)
    B = int(t.shape[0])
    if bool(xp.isnan(u).any()):
        raise ValueError(UPPER_NAN_MSG)
    if bool((u < 0).any()):
        raise ValueError(UPPER_NEG_MSG)
    fin = xp.isfinite(u)
    left = fin & (t == 0)
    if not bool((xp.isfinite(t) & ((t > 0) | left)).all()):
        raise ValueError(TIME_UPPER_MSG)
    ev = ~fin if event is None else _event_mask(event, B, xp, t)
    if bool((ev & fin).any()):
        raise ValueError(UPPER_EVENT_MSG)
    if bool((left & ~(u > 0)).any()):
        raise ValueError(UPPER_LEFT_MSG)
    itv = fin & ~left
    if bool((itv & ~(u > t)).any()):
        raise ValueError(UPPER_INTERVAL_MSG)
    zero = xp.zeros_like(t)
    y = xp.where(left, -u, xp.where(ev, t, -t))
    ud = xp.where(itv, u, xp.where(left, -u, zero))
    return y, ud


class WeibullReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: the state, the phases and the host views) with the shape k = e^tau and a
    response of three vectors -- time, event, upper -- packed into the signed y and the device encoding of the upper ends;
    params() reports shape_mean = E_q[k]."""
    link = "weibull"
    pass_name, finish_name = "bsc_glm_weibull_data_pass", "bsc_glm_weibull_update"
    scalar_attr, mean_key, prior_noun = "_logshape", "shape_mean", "the shape"
    has_exposure = False

    def __init__(self, X, time, event=None, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0,
                 b0=0.1, ctx=None, group=None, lam0=None, *, upper=None, offset=None, weights=None, covariance="diag"):
        """``time`` [B] finite and > 0; ``event`` [B] bool or 0/1, None = every row an event.  ``a0``, ``b0``: the
        Gamma(shape, rate) prior of the Weibull shape k (default: mean 10, wide).  ``lam0``: [m | rho] over
        [w (D) | tau] (default m = 0 -- tau starts at 0, k at 1, the exponential distribution -- and every rho = log 0.1).
        ``covariance``: "diag" (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the full
        layout, default the same start with no off-diagonal entries).  ``offset`` / ``weights``: float32 [B], as in
        GLMReparamSVI.  ``upper``: float [B] upper ends (module docstring; inf = none), None = the model without them.
        time, event, upper and the weights are checked here (one synchronisation), never in step()."""
        self._construct(X, (time, event, upper), n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group,
                        lam0, offset, weights, None, covariance)

    def _checked_response(self, time, event, upper):
        return pack_censored(time, event, upper)

    def _set_response(self, X, response, checked):
        y, u = pack_censored(*response) if checked is None else checked
        self._float_batch(X, y)
        self._set_upper(None if u is None else obs_vector(self.ctx, "upper", u, self.B))

    def _set_upper(self, upper):
        """The upper ends of the current batch in the device encoding: a tensor, a raw device pointer or None."""
        import torch
        self.upper = upper if isinstance(upper, torch.Tensor) else None
        self._uarg = upper if upper is None or isinstance(upper, torch.Tensor) else int(upper)

    def set_batch(self, X, time, event=None, rows=None, ldx=None, offset=None, weights=None, *, upper=None):
        """ReparamDriver.set_batch with the batch's censoring flags, offset and weights: tensors (time checked finite and
        > 0, event bool or 0/1, the weights finite and >= 0; y = where(event, time, -time) is what the driver keeps)
        with tensor X and time; raw device pointers (unchecked) with raw ones, ``time`` then being the signed vector and
        ``event`` not allowed.  ``upper``: the batch's upper ends (inf = none) with tensors; with raw pointers a raw pointer
        to the device encoding (pack_censored).  None drops offset, weights or upper for this batch."""
        import torch
        if isinstance(X, torch.Tensor):
            time, upper = pack_censored(time, event, upper)
            if upper is not None:
                upper = obs_vector(self.ctx, "upper", upper, X.shape[0])
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        elif event is not None:
            raise ValueError("with raw device pointers pass the signed vector where(event, time, -time) as time; "
                             "event= is for tensors")
        # (not ScalarLatentDriver.set_batch: that one checks a single y with check_response, which this family has not)
        ReparamDriver.set_batch(self, X, time, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)
        self._set_upper(upper)

    @property
    def logshape(self):
        return self._logshape[self.cur]

    # -- phases -------------------------------------------------------------------------------------------------
    def data_pass(self):
        if getattr(self, "_uarg", None) is None:
            return super().data_pass()
        # only a batch with upper ends takes the interval pass
        self.ctx.call("bsc_glm_weibull_data_pass_interval", self._Xarg, self._ldx, self._yarg, self._uarg, self._oarg,
                      self._varg, self.B, self.D, self.W, self.logshape, self.S, self.ell, self.G, self.T)

    # -- posterior predictive (svi/predict.py: one bsc_weibull_predict_pass over X for all draws) -------------------
    def _signed(self, time, event, upper=None):
        """The signed response of held-out rows and their upper ends in the device encoding (None without ``upper``), or
        (None, None) without ``time``."""
        if time is None:
            if event is not None:
                raise ValueError("event= needs time=")
            if upper is not None:
                raise ValueError("upper= needs time=")
            return None, None
        return pack_censored(time, event, upper)

    def predict(self, X, time=None, event=None, n_samples=64, seed=None, draws=None, offset=None, weights=None, *,
                upper=None):
        """``mean`` = E t and ``var`` = Var t per row under the posterior predictive and, with ``time``, ``lpd`` and
        ``lpd_sum``: the log predictive density at an event, the log predictive SURVIVAL probability at a censored
        time and, with ``upper``, the log predictive PROBABILITY of an interval or left-censored row."""
        from .predict import predict
        y, u = self._signed(time, event, upper)
        return predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights, upper=u)

    def heldout_lpd(self, X, time, event=None, n_samples=64, seed=None, draws=None, offset=None, weights=None, *,
                    upper=None):
        """Mean log predictive density per held-out row (a host float); with weights sum v lpd / sum v."""
        from .predict import heldout_lpd
        y, u = self._signed(time, event, upper)
        return heldout_lpd(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset, weights=weights,
                           upper=u)

    def survival(self, X, t, n_samples=64, seed=None, draws=None, offset=None):
        """S(t_n | x_n) = P(T_n > t_n) under the posterior predictive, float32 [B] on the device: one predictive pass with
        every row censored at t_n (its lpd is the log of the draw average of e^{-e^z}), exponentiated."""
        import torch
        from .predict import predict
        y = -pack_response(t)                     # t checked like a duration, every row censored
        return torch.exp(predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset)["lpd"])


check_arguments = WeibullReparamSVI.check_arguments
