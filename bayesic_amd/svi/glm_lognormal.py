"""Log-normal survival regression (accelerated failure time) with right censoring and a learned scale by
reparameterised-ELBO SVI on the fused pass.

Host-side driver of csrc/bsc_glm_lognormal.hip; every numeric step is a C-ABI call into libbayesic_hip.so.

Model:  t_n ~ LogNormal(location l_n, scale sigma),   l_n = x_n . w + o_n,   w ~ N(0, I / prior_precision),
        k = 1 / sigma = e^tau ~ Gamma(a0, b0);   delta_n = 1: the event was seen at t_n,  delta_n = 0: right-censored,
        the event is later than t_n.
q:      z = [w (D) | tau] ~ N(m, diag e^{2 rho}),  lam = [m (P) | rho (P)],  P = D + 1    (covariance="diag", default)
        z ~ N(mu, L L^T),  lam = [mu (P) | packed L]                                   (covariance="full", below).

The duration model that stands next to WeibullReparamSVI (svi/glm_weibull.py): a Weibull hazard is monotone, the
log-normal one rises and then falls (recovery times, time to relapse, repair times).  The two are fitted to the same
censored data and compared by heldout_lpd, which counts a censored held-out row through its predictive survival
probability in both.  The rows that are still running when the data are cut enter through log S(t) = log Phi(-z), the
others through the density, log f(t) = tau - log t - z^2 / 2 - log(2 pi) / 2, with z = k (log t - l).  Without
censoring this is a Gaussian regression of log t (Tobit on log t with it); dropping the censored rows, or treating the
cut-off as the event time, biases the location down and the scale with it.  l is the location of log t, the log
MEDIAN, not the log mean: E t = e^{l + sigma^2 / 2}, Var t = (e^{sigma^2} - 1) e^{2l + sigma^2}.

tau is the log of the INVERSE scale, not of sigma: the prior on e^tau then has the form the shared finish knows
(``a0``, ``b0`` are the Gamma(shape, rate) prior of 1 / sigma), and the finish is NegBinReparamSVI's.  The censoring
flag costs nothing on the device: the driver keeps ONE float32 vector y = where(event, time, -time)
(svi/glm_weibull.pack_response, the same packing and the same checks), and that vector is what the pass reads
(include/bayesic_hip.h, bsc_glm_lognormal_data_pass).  With raw device pointers the caller passes the signed vector.
The data enter one update through ell_s, G_s (svi/glm.py) and T_s = d ell_s / d tau_s, all from ONE streaming pass over
X; step() = pass -> all-reduce of [ell | G | T] -> bsc_glm_lognormal_update; the state, the first draw and step() are
ReparamDriver's (svi/_reparam_base.py), offsets and row weights svi/glm.py's (svi/_obs.py).  There is no ``exposure``: a
multiplier on the median has no established meaning here, and ``offset`` covers it.

``time`` must be finite and strictly positive, ``event`` a bool or 0/1 array of length B (None: every row is an event).
Both are checked where a batch is set -- the constructor and set_batch, on the host before a device is asked for when
they are host arrays -- and never in step(); raw device pointers are taken as they are.  The pass does not clamp and has
nothing to clamp: log Phi(-z) and the normal hazard come from one scaled complementary error function and are finite
and accurate in both tails (csrc/bsc_special_f32.h).

Accuracy envelope: tau in [-1.5, 4] (sigma from 4.5 down to 0.018); below it the predictive variance leaves float32
(e^{2 sigma^2} overflows at sigma^2 = 44, tau = -1.9).

``covariance="full"``: q(z) = N(mu, L L^T) over z = [w (D) | tau] in the full layout of svi/_reparam_base.py, first draw
mu + L eps, finish bsc_glm_scalar_fullrank_update (svi/glm_nb.py says more): no kernel of its own.  With censoring the
scale is correlated a posteriori with the intercept; a diagonal q reports it too narrow.

Out of scope, by design of this version: interval and left censoring (there is no ``upper=``; svi/glm_weibull.py has
them for its family); left truncation (delayed entry); random intercepts (svi/hier_scalar.py has no driver for this
family); recognition by ReparamVI (it does not recognise a log-normal log-joint); MiniBatchLoader (it does not carry
offset and weights).  There is no one-call (pass + finish) form, so every update is pass -> all-reduce -> finish.  The
multi-rank branch is wired like the other drivers' and has been exercised at world size 1 only.
"""
import math

from ._obs import batch_obs
from ._reparam_base import ReparamDriver
from ._scalar_latent import ScalarLatentDriver
from .glm_weibull import pack_response


class LogNormalReparamSVI(ScalarLatentDriver):
    """ScalarLatentDriver (svi/_scalar_latent.py: the state, the phases and the host views) with the inverse scale
    k = 1 / sigma = e^tau and a response of two vectors -- time, event -- packed into the signed y; params() reports
    inv_sigma_mean = E_q[1 / sigma] and sigma_mean = E_q[sigma]."""
    link = "lognormal"
    pass_name, finish_name = "bsc_glm_lognormal_data_pass", "bsc_glm_lognormal_update"
    scalar_attr, mean_key, prior_noun = "_loginvscale", "inv_sigma_mean", "the inverse scale"
    has_exposure = False

    def __init__(self, X, time, event=None, n_total=None, n_samples=8, seed=1234, lr=1e-2, prior_precision=1.0, a0=1.0,
                 b0=0.1, ctx=None, group=None, lam0=None, *, offset=None, weights=None, covariance="diag"):
        """``time`` [B] finite and > 0; ``event`` [B] bool or 0/1, None = every row an event.  ``a0``, ``b0``: the
        Gamma(shape, rate) prior of the inverse scale 1 / sigma (default: mean 10, wide).  ``lam0``: [m | rho] over
        [w (D) | tau] (default m = 0 -- tau starts at 0, sigma at 1 -- and every rho = log 0.1).  ``covariance``: "diag"
        (the mean-field guide, default) or "full" (module docstring; ``lam0`` then in the full layout, default the same
        start with no off-diagonal entries).  ``offset`` / ``weights``: float32 [B], as in GLMReparamSVI.  time, event
        and the weights are checked here (one synchronisation), never in step()."""
        self._construct(X, (time, event), n_total, n_samples, seed, lr, prior_precision, a0, b0, ctx, group, lam0,
                        offset, weights, None, covariance)

    def _checked_response(self, time, event):
        return pack_response(time, event)

    def _set_response(self, X, response, checked):
        self._float_batch(X, pack_response(*response) if checked is None else checked)

    def set_batch(self, X, time, event=None, rows=None, ldx=None, offset=None, weights=None):
        """ReparamDriver.set_batch with the batch's censoring flags, offset and weights: tensors (time checked finite and
        > 0, event bool or 0/1, the weights finite and >= 0; y = where(event, time, -time) is what the driver keeps)
        with tensor X and time; raw device pointers (unchecked) with raw ones, ``time`` then being the signed vector and
        ``event`` not allowed.  None drops offset or weights for this batch."""
        import torch
        if isinstance(X, torch.Tensor):
            time = pack_response(time, event)
            offset, weights = batch_obs(self.ctx, X.shape[0], offset, weights)
        elif event is not None:
            raise ValueError("with raw device pointers pass the signed vector where(event, time, -time) as time; "
                             "event= is for tensors")
        # (not ScalarLatentDriver.set_batch: that one checks a single y with check_response, which this family has not)
        ReparamDriver.set_batch(self, X, time, rows=rows, ldx=ldx)
        self._set_obs(offset, weights)

    @property
    def loginvscale(self):
        return self._loginvscale[self.cur]

    # -- posterior predictive (svi/predict.py: one bsc_lognormal_predict_pass over X for all draws) -------------------
    def _signed(self, time, event):
        """The signed response of held-out rows, or None without ``time``."""
        if time is None:
            if event is not None:
                raise ValueError("event= needs time=")
            return None
        return pack_response(time, event)

    def predict(self, X, time=None, event=None, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """``mean`` = E t and ``var`` = Var t per row under the posterior predictive and, with ``time``, ``lpd`` and
        ``lpd_sum``: the log predictive density at an event, the log predictive SURVIVAL probability at a censored
        time."""
        from .predict import predict
        return predict(self, X, self._signed(time, event), n_samples=n_samples, seed=seed, draws=draws, offset=offset,
                       weights=weights)

    def heldout_lpd(self, X, time, event=None, n_samples=64, seed=None, draws=None, offset=None, weights=None):
        """Mean log predictive density per held-out row (a host float); with weights sum v lpd / sum v."""
        from .predict import heldout_lpd
        return heldout_lpd(self, X, self._signed(time, event), n_samples=n_samples, seed=seed, draws=draws,
                           offset=offset, weights=weights)

    def survival(self, X, t, n_samples=64, seed=None, draws=None, offset=None):
        """S(t_n | x_n) = P(T_n > t_n) under the posterior predictive, float32 [B] on the device: one predictive pass with
        every row censored at t_n (its lpd is the log of the draw average of Phi(-z)), exponentiated."""
        import torch
        from .predict import predict
        y = -pack_response(t)                     # t checked like a duration, every row censored
        return torch.exp(predict(self, X, y, n_samples=n_samples, seed=seed, draws=draws, offset=offset)["lpd"])

    # -- host views -----------------------------------------------------------------------------------------------
    def params(self):
        """ScalarLatentDriver.params() -- inv_sigma_mean = E_q[e^tau] = exp(m_tau + Var_q(tau) / 2) -- and sigma_mean =
        E_q[e^{-tau}] = exp(-m_tau + Var_q(tau) / 2), with the marginal variance of tau under the full guide."""
        out = super().params()
        out["sigma_mean"] = out["inv_sigma_mean"] * math.exp(-2.0 * float(out["tau"][0]))
        return out


check_arguments = LogNormalReparamSVI.check_arguments
