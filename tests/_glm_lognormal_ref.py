"""Float64 numpy restatement of the log-normal survival route (include/bayesic_hip.h: bsc_glm_lognormal_data_pass,
bsc_glm_lognormal_update, bsc_lognormal_predict_pass; svi/glm_lognormal.py):

    t_n ~ LogNormal(location l, scale sigma),  l[n,s] = x_n . w_s + o_n,  k_s = 1 / sigma_s = e^{tau_s}
    y_n > 0: an event at y_n (delta = 1);  y_n < 0: right-censored at -y_n (delta = 0);  t = |y|, ly = log t
    z = k (ly - l),   log f = tau - ly - z^2 / 2 - log(2 pi) / 2,   log S = log Phi(-z),   h(z) = phi(z) / Phi(-z)
    ell[s] = sum_n v_n [ delta_n log f + (1 - delta_n) log Phi(-z_ns) ]
    r[n,s] = v_n k_s [ delta_n z_ns + (1 - delta_n) h(z_ns) ],   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n [ delta_n (1 - z_ns^2) - (1 - delta_n) z_ns h(z_ns) ]

under w ~ N(0, I / prec), k ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select, whatever they hold.  The prior on e^tau has the negative binomial's form, so the draws, the
finish and the stepper's Adam are tests/_glm_nb_ref.py's by import (log(1 / sigma) in the place of log phi); the logits
come from tests/_glm_obs_ref.py.  log Phi(-z) is scipy's log_ndtr, and h = exp(log phi(z) - log Phi(-z)): neither tail
cancels or overflows in float64.

The bound quantities (``bounds``, ``predict_bounds``) are tests/_glm_weibull_ref.py's construction: the sums of the
absolute sizes of the terms, with the conditioning of z on its rounded inputs.  z = k (ly - l) is formed in float32
from a rounded k, a rounded ly and a logit whose float32 terms have the size a = sum_d |x_d w_d| + |o|, so its absolute
error is a multiple of eps times c = |z| + k (|ly| + a); the derivative of z^2 / 2 is z, of log Phi(-z) it is -h, of h
it is h (h - z), of z h it is h + z h (h - z).  Per kept (row, draw), times the weight:
    ell:  delta (|tau| + |ly| + z^2 / 2 + |z| c + 1) + (1 - delta)(|log Phi(-z)| + h c + 1)
    r:    k [ delta (|z| + c) + (1 - delta) h (1 + |h - z| c) ]
    T:    delta (1 + z^2 + 2 |z| c) + (1 - delta)(|z| h + (h + |z| h |h - z|) c) + 1
A device result is held to EPS = 2e-5 times these, a plain float32 replay of the device's forms to 1e-6 times these
(tests/test_glm_lognormal_cpu.py), as tests/_glm_weibull_ref.py holds its model."""
import math

import numpy as np
from scipy.special import log_ndtr

import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

LOG_2PI = nb.LOG_2PI
EPS = 2e-5
TAU_LO, TAU_HI = -1.5, 4.0       # the accuracy envelope (include/bayesic_hip.h)
Z_MAX = 60.0
_f64 = obs._f64


def log_sf_hazard(z):
    """(log Phi(-z), phi(z) / Phi(-z)) in float64, stable in both tails."""
    z = np.asarray(z, np.float64)
    lsf = log_ndtr(-z)
    return lsf, np.exp(-0.5 * z * z - 0.5 * LOG_2PI - lsf)


# ---- inputs shared by tests/test_glm_lognormal_cpu.py and tests/test_glm_lognormal_gpu.py -------------------------------

def make_inputs(B, D, S, seed, mode="both", censored=0.3, z_max=Z_MAX, tau=None):
    """tests/_glm_weibull_ref.make_inputs' recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every
    fifth exactly zero) with tau spread over the accuracy envelope [-1.5, 4] (``tau``: given) and durations drawn from
    LogNormal(l, 0.7) at the first draw's logit.  A share ``censored`` of the rows is cut at a uniform fraction of its
    duration and flagged by a negative y (0.0: every row an event, 1.0: every row censored).
    |z| = k |log t - l| <= z_max for every kept (row, draw) needs more than one factor on the durations here, because
    both tails count: a row's log t has to lie within z_max / k_s of EVERY draw's logit, and at k = e^4 that is 1.1.  So
    (1) the draws' weights are pulled towards the first draw's by one factor gamma <= 1, W_s = W_0 + gamma (W_s - W_0),
    the largest at which every kept row has such a log t (the logits of two draws differ by gamma x_n . (W_s - W_s'),
    which must not exceed z_max (1 / k_s + 1 / k_s')); (2) each row's log t is clipped into the interval that is left.
    With weights, the rows of weight 0 hold y = 0 and y = NaN in turn.
    Returns (X, y signed, W, loginvscale, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o, use_v = mode in ("offset", "both"), mode in ("weights", "both")
    if tau is None:
        lis = np.linspace(TAU_LO, TAU_HI, S)[rs.permutation(S)] if S > 1 else np.array([0.5])
    else:
        lis = np.broadcast_to(np.asarray(tau, np.float64), (S,))
    lis = lis.astype(np.float32)
    k = np.exp(_f64(lis))[None, :]
    keep = (v > 0) if use_v else np.ones(B, bool)
    room = 0.98 * z_max / k                                      # [1, S]: how far log t may lie from a draw's logit
    L = obs.logits(X, W, None)
    gap = np.abs(L[keep][:, :, None] - L[keep][:, None, :])      # [kept, S, S']
    need = 1.001 * (gap / (room[0][None, :, None] + room[0][None, None, :])).max()    # (W is rounded again below)
    if need > 1.0:
        W = (_f64(W[0])[None, :] + (_f64(W) - _f64(W[0])[None, :]) / need).astype(np.float32)
    L = obs.logits(X, W, o if use_o else None)
    t = np.exp(L[:, 0] + 0.7 * rs.standard_normal(B))
    cens = rs.uniform(size=B) < censored
    t = np.where(cens, t * rs.uniform(0.1, 1.0, B), t)
    y = refit(np.where(cens, -t, t), L, lis, keep, z_max)
    if use_v:
        dead = np.flatnonzero(v == 0)
        y[dead[0::2]] = 0.0
        y[dead[1::2]] = np.nan
    return X, y, W, lis, (o if use_o else None), (v if use_v else None)


def refit(y, L, loginvscale, keep=None, z_max=Z_MAX):
    """The signed durations y with each kept row's log t clipped into the interval where |z| <= z_max at every draw of
    the logits L [B, S] (0.98 z_max before the rounding to float32); a kept row without such an interval is an error."""
    k = np.exp(_f64(loginvscale))[None, :]
    keep = np.ones(L.shape[0], bool) if keep is None else keep
    room = 0.98 * z_max / k
    lo, hi = (L - room).max(axis=1), (L + room).min(axis=1)
    assert (lo[keep] <= hi[keep]).all()
    ly = np.log(np.abs(_f64(y)))
    ly = np.where(keep, np.clip(ly, lo, hi), ly)
    out = (np.sign(y) * np.exp(ly)).astype(np.float32)
    z = k * (np.log(np.abs(_f64(out)))[:, None] - L)
    assert np.abs(z[keep]).max() <= z_max
    return out


def make_pinned(B, D, S, seed, tau=1.0, z_pin=Z_MAX):
    """Every row censored with z pinned at +z_pin and -z_pin in turn, at every draw: one tau and one weight vector for
    all S draws (so that the logit of a row is the same at every draw), log t = l +- z_pin / k.  Offsets and weights as
    in make_inputs.  Returns (X, y, W, loginvscale, offset, weights)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = np.repeat((0.6 * rs.standard_normal((1, D))).astype(np.float32), S, axis=0)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    lis = np.full(S, tau, np.float32)
    L = obs.logits(X, W, o)[:, 0]
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0)
    y = (-np.exp(L + sign * z_pin / math.exp(float(lis[0])))).astype(np.float32)
    return X, y, W, lis, o, v


# ---- the pass -------------------------------------------------------------------------------------------------------

def logit_size(X, W, offset):
    """a[n,s] = sum_d |x_nd w_sd| + |o_n|: the size of the logit's float32 terms."""
    a = np.abs(_f64(X)) @ np.abs(_f64(W)).T
    return a if offset is None else a + np.abs(_f64(offset))[:, None]


def _terms(X, y, W, loginvscale, offset, weights):
    """Per (row, draw): the terms of ell, the residual, the terms of T, and the three bound quantities."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    y64 = _f64(y)[:, None]
    tau = _f64(loginvscale)[None, :]
    k = np.exp(tau)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        dl = (y64 > 0).astype(np.float64)
        ly = np.log(np.abs(y64))
        z = k * (ly - L)
        az = np.abs(z)
        lsf, h = log_sf_hazard(z)
        c = az + k * (np.abs(ly) + a)
        t_ell = np.where(on, vv * np.where(dl > 0, tau - ly - 0.5 * z * z - 0.5 * LOG_2PI, lsf), 0.0)
        a_ell = np.where(on, vv * np.where(dl > 0, np.abs(tau) + np.abs(ly) + 0.5 * z * z + az * c + 1.0,
                                           np.abs(lsf) + h * c + 1.0), 0.0)
        r = np.where(on, vv * k * np.where(dl > 0, z, h), 0.0)
        a_r = np.where(on, vv * k * np.where(dl > 0, az + c, h * (1.0 + np.abs(h - z) * c)), 0.0)
        t_T = np.where(on, vv * np.where(dl > 0, 1.0 - z * z, -z * h), 0.0)
        a_T = np.where(on, vv * (np.where(dl > 0, 1.0 + z * z + 2.0 * az * c,
                                          az * h + (h + az * h * np.abs(h - z)) * c) + 1.0), 0.0)
    return t_ell, a_ell, r, a_r, t_T, a_T


def data_pass(X, y, W, loginvscale, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, _, t_T, _ = _terms(X, y, W, loginvscale, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, loginvscale, offset=None, weights=None):
    """(b_ell [S], b_G [S, D], b_T [S]): what the errors are measured against (module docstring), rows of weight 0 left
    out; b_G[s,d] = sum_n a_r[n,s] |x_nd|."""
    _, a_ell, _, a_r, _, a_T = _terms(X, y, W, loginvscale, offset, weights)
    return a_ell.sum(axis=0), a_r.T @ np.abs(_f64(X)), a_T.sum(axis=0)


def row_logpdf(L, y, loginvscale):
    """log f(|y|) where y > 0 and log S(|y|) where y < 0, per (row, draw): [B, S]."""
    y64 = _f64(y)[:, None]
    tau = _f64(loginvscale)[None, :]
    ly = np.log(np.abs(y64))
    z = np.exp(tau) * (ly - L)
    return np.where(y64 > 0, tau - ly - 0.5 * z * z - 0.5 * LOG_2PI, log_ndtr(-z))


# ---- the device's forms in plain float32 ----------------------------------------------------------------------------------

ERFCX_COEF = (6.807514728279784e-05, 1.6084033995866776e-04, -3.709284064825624e-04, -1.3958050403743982e-03,
              1.230503199622035e-03, 8.68925265967846e-03, -8.024739101529121e-03, -5.4211996495723724e-02,
              1.6405050456523895e-01, -1.660310924053192e-01, -9.276381880044937e-02, 2.7697840332984924e-01)


def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two float32 values is exact in float64, the sum is rounded once there and
    once more to float32."""
    return (_f64(a) * _f64(b) + _f64(c)).astype(np.float32)


def erfcx_pos_f32(a):
    """csrc/bsc_special_f32.h's bsc_erfcx_pos_f32 replayed in float32, step by step with its coefficients (highest degree
    first); the two hardware reciprocals are 1 / x rounded to float32."""
    f = np.float32
    a = np.asarray(a, f)
    r2 = f(1.0) / (a + f(2.0))
    t0 = (a - f(2.0)) * r2
    t = _fma(r2, _fma(t0, -a, _fma(t0 + f(1.0), f(-2.0), a)), t0)
    p = np.full_like(a, f(ERFCX_COEF[0]))
    for c in ERFCX_COEF[1:]:
        p = _fma(p, t, f(c))
    r = f(0.5) * (f(1.0) / (a + f(0.5)))
    q = _fma(p, r, r)
    out = _fma((p - q) + _fma(q + q, -a, f(1.0)), r, q)
    assert out.dtype == f
    return out


def log_sf_hazard_f32(z):
    """csrc/bsc_special_f32.h's bsc_lognormsf_hazard_f32 in plain float32, erfcx_pos_f32 above for the device's:
    E = erfcx(|z| / sqrt 2); z >= 0: lsf = -z^2 / 2 + log(E / 2), h = sqrt(2 / pi) / E; z < 0: q = g E / 2 with
    g = e^{-z^2 / 2} corrected for the rounding of z^2 / 2, lsf = log(w) q / (1 - w) with w = 1 - q (-q where w == 1),
    h = phi(z) / w."""
    f = np.float32
    z = np.asarray(z, f)
    pos = z >= 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        E = erfcx_pos_f32(np.abs(z) * f(0.70710678118654752))
        hz2 = f(0.5) * z * z
        g0 = np.exp(-hz2)
        d = _fma(f(0.5) * z, z, -hz2)                # the rounding error of hz2, exact
        g = _fma(-g0, d, g0)
        q = f(0.5) * g * E
        w = f(1.0) - q
        tiny = ~pos & (w == 1)
        lg = np.log(np.where(pos, f(0.5) * E, w))
        ratio = np.where(pos, f(1.0), q * (f(1.0) / np.where(tiny, f(1.0), f(1.0) - w)))
        lsf = lg * ratio + np.where(tiny, -q, np.where(pos, -hz2, f(0.0)))
        h = np.where(pos, f(0.79788456080286536), f(0.39894228040143268) * g) * (f(1.0) / np.where(pos, E, w))
    assert lsf.dtype == f and h.dtype == f
    return lsf, h


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def data_pass_f32(X, y, W, loginvscale, offset=None, weights=None):
    """The same formulas evaluated plainly in float32 in the order of csrc/bsc_families.h's link, the logits by one
    float32 matrix product, float32 partials of F32_BLOCK rows finished in float64
    (tests/_glm_weibull_ref.data_pass_f32)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, loginvscale))
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
        cs = one - dl
        z = k[None, :] * (ly - np.where(keep[:, None], l, f(0.0)))
        lsf, h = log_sf_hazard_f32(z)
        zz = z * z
        t_ell = vq * (dl * ((tau[None, :] - ly) - (f(0.5) * zz + f(0.5 * LOG_2PI))) + cs * lsf)
        t_T = vq * (dl * (one - zz) - cs * (z * h))
        r = vq * (k[None, :] * (dl * z + cs * h))
    assert t_ell.dtype == f and t_T.dtype == f and r.dtype == f and l.dtype == f
    ell, G, T = np.zeros(S), np.zeros((S, D)), np.zeros(S)
    for b in range(0, B, F32_BLOCK):
        ell += np.cumsum(t_ell[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        T += np.cumsum(t_T[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        G += np.cumsum(r[b:b + F32_BLOCK, :, None] * X[b:b + F32_BLOCK, None, :], axis=0, dtype=f)[-1]
    return ell, G, T


# ---- draws and the finish: the negative binomial's (the scalar's prior has the same form) ---------------------------------

init_lam = nb.init_lam              # m = 0 (tau = 0, sigma = 1), rho = log 0.1
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1]
draw = nb.draw                      # (W [S, D] float32, loginvscale [S] float32)
log_prior_tau = nb.log_prior_tau
elbo_and_grad = nb.elbo_and_grad    # (lam, eps, W, loginvscale, ell, G, T, scale, prec, a0, b0)
update = nb.finish                  # bsc_glm_lognormal_update from given statistics: (lam', m1', m2', elbo, grad)


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as LogNormalReparamSVI does it;
    y is the signed response."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, lis = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, lis, offset, weights)
    return update(lam, m1, m2, t, eps, W, lis, ell, G, T, n_total / B, prec, a0, b0, lr)


def elbo_terms_size(W, loginvscale, ell_bound, scale, prec=1.0, a0=1.0, b0=1.0, rho=None):
    """The sum of the absolute values of the ELBO's terms, from reference quantities alone (tests/_glm_gamma_ref.py)."""
    w, tau = np.asarray(W, np.float64), np.asarray(loginvscale, np.float64)
    D = w.shape[1]
    P = D + 1
    per_draw = scale * ell_bound + 0.5 * prec * (w * w).sum(axis=1) + np.abs(a0 * tau) + b0 * np.exp(tau)
    const = abs(0.5 * D * math.log(prec / (2.0 * math.pi))) + abs(a0 * math.log(b0) - math.lgamma(a0))
    return per_draw.mean() + const + np.abs(rho).sum() + 0.5 * P * (1.0 + LOG_2PI)


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], loginvscale float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def moment_constants(tau):
    """m1 = e^{sigma^2 / 2} and m2 = (e^{sigma^2} - 1) e^{sigma^2}, sigma^2 = e^{-2 tau}: E t = e^l m1,
    Var t = e^{2l} m2."""
    s2 = np.exp(-2.0 * np.asarray(tau, np.float64))
    return np.exp(0.5 * s2), np.expm1(s2) * np.exp(s2)


def _lse_mean(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(X, W, loginvscale, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with the signed y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    g1, g2 = moment_constants(_f64(loginvscale)[None, :])
    mu = np.exp(L) * g1
    v = np.exp(2.0 * L) * g2
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = _lse_mean(row_logpdf(L, y, loginvscale))
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def survival(X, W, loginvscale, t, offset=None):
    """S(t_n | x_n) = mean_s Phi(-z_ns): [B]."""
    L = obs.logits(X, W, offset)
    z = np.exp(_f64(loginvscale))[None, :] * (np.log(_f64(t))[:, None] - L)
    return np.exp(log_ndtr(-z)).mean(axis=1)


def predict_bounds(X, W, loginvscale, y=None, offset=None, weights=None):
    """tests/_glm_weibull_ref.predict_bounds' construction for this family.  With a = logit_size and EPS = 2e-5:
    mu = e^l m1, d mu / d l = mu: e_mu = EPS (mu a + mu), the second term covering the float32 m1;  v = e^{2l} m2,
    dv/dl = 2 v: e_v = EPS (2 v a + v);  log p: EPS times the pass's per-row ell quantity (module docstring), maximum
    over the draws."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    tau = _f64(loginvscale)[None, :]
    k = np.exp(tau)
    g1, g2 = moment_constants(tau)
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
        ly = np.log(np.abs(y64))
        z = k * (ly - L)
        az = np.abs(z)
        lsf, h = log_sf_hazard(z)
        c = az + k * (np.abs(ly) + a)
        e = EPS * np.where(y64 > 0, np.abs(tau) + np.abs(ly) + 0.5 * z * z + az * c + 1.0, np.abs(lsf) + h * c + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
