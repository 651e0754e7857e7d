"""Float64 numpy restatement of the Weibull survival route (include/bayesic_hip.h: bsc_glm_weibull_data_pass,
bsc_glm_weibull_update, bsc_weibull_predict_pass; svi/glm_weibull.py):

    t_n ~ Weibull(shape k, scale e^l),  l[n,s] = x_n . w_s + o_n,  k_s = e^{tau_s}
    y_n > 0: an event at y_n (delta = 1);  y_n < 0: right-censored at -y_n (delta = 0);  t = |y|, ly = log t
    z = k (ly - l),   log f = tau + z - ly - e^z,   log S = -e^z
    ell[s] = sum_n v_n [ delta_n (tau_s + z_ns - ly_n) - e^{z_ns} ]
    r[n,s] = v_n k_s (e^{z_ns} - delta_n),   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n [ delta_n (1 + z_ns) - z_ns e^{z_ns} ]

under w ~ N(0, I / prec), k ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select, whatever they hold.  The prior on the scalar has the negative binomial's form, so the draws,
the finish and the stepper's Adam are tests/_glm_nb_ref.py's by import (log k in the place of log phi); the logits come
from tests/_glm_obs_ref.py.

The bound quantities (``bounds``, ``predict_bounds``) are the sums of the absolute sizes of the terms, with the
conditioning of z on its rounded inputs: z = k (ly - l) is formed in float32 BEFORE the exponential, from a rounded k,
a rounded ly and a logit whose float32 terms have the size a = sum_d |x_d w_d| + |o|, so its absolute error is a
multiple of eps times c = |z| + k (|ly| + a), and that costs c eps of e^z.  Per kept (row, draw):
    ell:  delta (|tau| + |z| + |ly| + c) + (1 + c) e^z + 1            (holds the (1 + |z|) e^z of the rounded argument)
    r:    k ( (1 + c) e^z + delta )
    T:    delta (1 + |z| + c) + (|z| + (1 + |z|) c) e^z + 1           (d/dz of z e^z is (1 + z) e^z)
A device result is held to EPS = 2e-5 times these, a plain float32 evaluation to 1e-6 times these
(tests/test_glm_weibull_cpu.py), as tests/_glm_gamma_ref.py holds its model."""
import math

import numpy as np
from scipy.special import gammaln

import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

LOG_2PI = nb.LOG_2PI
EPS = 2e-5
TAU_LO, TAU_HI = -2.0, 4.0       # the accuracy envelope (include/bayesic_hip.h)
_f64 = obs._f64


# ---- inputs shared by tests/test_glm_weibull_cpu.py and tests/test_glm_weibull_gpu.py ------------------------------------

def make_inputs(B, D, S, seed, mode="both", censored=0.3, z_max=60.0, tau=None):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every fifth
    exactly zero) with tau spread over the accuracy envelope [-2, 4] (``tau``: given) and durations drawn from
    Weibull(shape 1.5, scale e^l) at the first draw's logit.  A share ``censored`` of the rows is cut at a uniform
    fraction of its duration and flagged by a negative y (0.0: every row an event, 1.0: every row censored).  All
    durations are then scaled by one factor so that z = k (log t - l) <= z_max for every kept (row, draw): the link is
    not clamped.  With weights, the rows of weight 0 hold y = 0 and y = NaN in turn.
    Returns (X, y signed, W, logshape, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o, use_v = mode in ("offset", "both"), mode in ("weights", "both")
    L = obs.logits(X, W, o if use_o else None)
    t = np.exp(L[:, 0]) * rs.weibull(1.5, B)
    cens = rs.uniform(size=B) < censored
    t = np.where(cens, t * rs.uniform(0.1, 1.0, B), t)
    t = np.maximum(t, 1.0e-30)
    if tau is None:
        logshape = np.linspace(TAU_LO, TAU_HI, S)[rs.permutation(S)] if S > 1 else np.array([0.5])
    else:
        logshape = np.broadcast_to(np.asarray(tau, np.float64), (S,))
    logshape = logshape.astype(np.float32)
    k = np.exp(_f64(logshape))[None, :]
    keep = (v > 0) if use_v else np.ones(B, bool)
    over = (np.log(t)[:, None] - L - z_max / k)[keep].max()
    t = t * math.exp(-max(over, 0.0) - 1e-3)
    y = np.where(cens, -t, t).astype(np.float32)
    if use_v:
        dead = np.flatnonzero(v == 0)
        y[dead[0::2]] = 0.0
        y[dead[1::2]] = np.nan
    return X, y, W, logshape, (o if use_o else None), (v if use_v else None)


# ---- the pass -------------------------------------------------------------------------------------------------------

def logit_size(X, W, offset):
    """a[n,s] = sum_d |x_nd w_sd| + |o_n|: the size of the logit's float32 terms."""
    a = np.abs(_f64(X)) @ np.abs(_f64(W)).T
    return a if offset is None else a + np.abs(_f64(offset))[:, None]


def _terms(X, y, W, logshape, offset, weights):
    """Per (row, draw): the terms of ell, the residual, the terms of T, and the three bound quantities."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    y64 = _f64(y)[:, None]
    tau = _f64(logshape)[None, :]
    k = np.exp(tau)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        dl = (y64 > 0).astype(np.float64)
        ly = np.log(np.abs(y64))
        z = k * (ly - L)
        ez = np.exp(z)
        az = np.abs(z)
        c = az + k * (np.abs(ly) + a)
        t_ell = np.where(on, vv * (dl * (tau + z - ly) - ez), 0.0)
        a_ell = np.where(on, vv * (dl * (np.abs(tau) + az + np.abs(ly) + c) + (1.0 + c) * ez + 1.0), 0.0)
        r = np.where(on, vv * k * (ez - dl), 0.0)
        a_r = np.where(on, vv * k * ((1.0 + c) * ez + dl), 0.0)
        t_T = np.where(on, vv * (dl * (1.0 + z) - z * ez), 0.0)
        a_T = np.where(on, vv * (dl * (1.0 + az + c) + (az + (1.0 + az) * c) * ez + 1.0), 0.0)
    return t_ell, a_ell, r, a_r, t_T, a_T


def data_pass(X, y, W, logshape, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, _, t_T, _ = _terms(X, y, W, logshape, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, logshape, offset=None, weights=None):
    """(b_ell [S], b_G [S, D], b_T [S]): what the errors are measured against (module docstring), rows of weight 0 left
    out; b_G[s,d] = sum_n a_r[n,s] |x_nd|."""
    _, a_ell, _, a_r, _, a_T = _terms(X, y, W, logshape, offset, weights)
    return a_ell.sum(axis=0), a_r.T @ np.abs(_f64(X)), a_T.sum(axis=0)


def row_logpdf(L, y, logshape):
    """log f(|y|) where y > 0 and log S(|y|) where y < 0, per (row, draw): [B, S]."""
    y64 = _f64(y)[:, None]
    tau = _f64(logshape)[None, :]
    ly = np.log(np.abs(y64))
    z = np.exp(tau) * (ly - L)
    return np.where(y64 > 0, tau + z - ly - np.exp(z), -np.exp(z))


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def data_pass_f32(X, y, W, logshape, offset=None, weights=None):
    """The same formulas evaluated plainly in float32 (every row at once: numpy keeps float32 arrays in float32), in the
    order of csrc/bsc_glm_pass.h's link, the logits by one float32 matrix product.  The sums follow the pass's design,
    float32 partials finished in float64: F32_BLOCK rows are added one after the other in float32 (a cumulative sum),
    the partials in float64 (tests/_glm_gamma_ref.data_pass_f32 says why: one float32 sum over all rows would measure
    its own length, not the formulas)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, logshape))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    k = np.exp(tau)
    one = f(1.0)
    keep = v > 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # every array below is float32
        l = X @ W.T + o[:, None]
        vq = np.where(keep, v, f(0.0))[:, None]             # the selects sit on the inputs, as in the link
        ly = np.log(np.where(keep, np.abs(y), one))[:, None]
        dl = np.where(keep & (y > 0), one, f(0.0))[:, None]
        z = k[None, :] * (ly - np.where(keep[:, None], l, f(0.0)))
        ez = np.exp(z)
        t_ell = vq * (dl * ((tau[None, :] + z) - ly) - ez)
        t_T = vq * (dl * (one + z) - z * ez)
        r = vq * (k[None, :] * (ez - dl))
    assert t_ell.dtype == f and t_T.dtype == f and r.dtype == f and l.dtype == f
    ell, G, T = np.zeros(S), np.zeros((S, D)), np.zeros(S)
    for b in range(0, B, F32_BLOCK):
        ell += np.cumsum(t_ell[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        T += np.cumsum(t_T[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        G += np.cumsum(r[b:b + F32_BLOCK, :, None] * X[b:b + F32_BLOCK, None, :], axis=0, dtype=f)[-1]
    return ell, G, T


# ---- draws and the finish: the negative binomial's (the scalar's prior has the same form) ---------------------------------

init_lam = nb.init_lam              # m = 0 (tau = 0), rho = log 0.1
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1]
draw = nb.draw                      # (W [S, D] float32, logshape [S] float32)
log_prior_tau = nb.log_prior_tau
elbo_and_grad = nb.elbo_and_grad    # (lam, eps, W, logshape, ell, G, T, scale, prec, a0, b0)
update = nb.finish                  # bsc_glm_weibull_update from given statistics: (lam', m1', m2', elbo, grad)


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as WeibullReparamSVI does it;
    y is the signed response."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logshape = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, logshape, offset, weights)
    return update(lam, m1, m2, t, eps, W, logshape, ell, G, T, n_total / B, prec, a0, b0, lr)


def elbo_terms_size(W, logshape, ell_bound, scale, prec=1.0, a0=1.0, b0=1.0, rho=None):
    """The sum of the absolute values of the ELBO's terms, from reference quantities alone (tests/_glm_gamma_ref.py)."""
    w, tau = np.asarray(W, np.float64), np.asarray(logshape, np.float64)
    D = w.shape[1]
    P = D + 1
    per_draw = scale * ell_bound + 0.5 * prec * (w * w).sum(axis=1) + np.abs(a0 * tau) + b0 * np.exp(tau)
    const = abs(0.5 * D * math.log(prec / (2.0 * math.pi))) + abs(a0 * math.log(b0) - math.lgamma(a0))
    return per_draw.mean() + const + np.abs(rho).sum() + 0.5 * P * (1.0 + LOG_2PI)


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], logshape float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def moment_constants(k):
    """g1 = Gamma(1 + 1/k) and g2 = Gamma(1 + 2/k) - Gamma(1 + 1/k)^2: E t = e^l g1, Var t = e^{2l} g2."""
    g1 = np.exp(gammaln(1.0 + 1.0 / k))
    return g1, np.exp(gammaln(1.0 + 2.0 / k)) - g1 * g1


def _lse_mean(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(X, W, logshape, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with the signed y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    g1, g2 = moment_constants(np.exp(_f64(logshape))[None, :])
    mu = np.exp(L) * g1
    v = np.exp(2.0 * L) * g2
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = _lse_mean(row_logpdf(L, y, logshape))
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def survival(X, W, logshape, t, offset=None):
    """S(t_n | x_n) = mean_s exp(-e^{z_ns}): [B]."""
    L = obs.logits(X, W, offset)
    z = np.exp(_f64(logshape))[None, :] * (np.log(_f64(t))[:, None] - L)
    return np.exp(-np.exp(z)).mean(axis=1)


def predict_bounds(X, W, logshape, y=None, offset=None, weights=None):
    """tests/_glm_gamma_ref.predict_bounds' construction for this family.  With a = logit_size and EPS = 2e-5:
    mu = e^l g1, d mu / d l = mu: e_mu = EPS (mu a + mu), the second term covering the float32 g1;  v = e^{2l} g2,
    dv/dl = 2 v: e_v = EPS (2 v a + v);  log p: EPS times the pass's per-row ell quantity (module docstring), maximum
    over the draws."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    tau = _f64(logshape)[None, :]
    k = np.exp(tau)
    g1, g2 = moment_constants(k)
    mu = np.exp(L) * g1
    v = np.exp(2.0 * L) * g2
    e_mu = EPS * (mu * a + mu)
    e_v = EPS * (2.0 * v * a + v)
    mean = mu.mean(axis=1)
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = _f64(y)[:, None]
        dl = (y64 > 0).astype(np.float64)
        ly = np.log(np.abs(y64))
        z = k * (ly - L)
        az = np.abs(z)
        c = az + k * (np.abs(ly) + a)
        e = EPS * (dl * (np.abs(tau) + az + np.abs(ly) + c) + (1.0 + c) * np.exp(z) + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
