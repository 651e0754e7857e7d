"""Float64 numpy restatement of the Gamma route (include/bayesic_hip.h: bsc_glm_gamma_data_pass, bsc_glm_gamma_update,
bsc_gamma_predict_pass; svi/glm_gamma.py):

    y_n ~ Gamma(shape alpha, rate alpha / mu_n),  mu = e^l,  l[n,s] = x_n . w_s + o_n,  alpha_s = e^{tau_s}
    ly = log y,  c_a = alpha log alpha - lnGamma(alpha),  c_1 = log alpha + 1 - psi(alpha)
    log p(y | l, alpha) = c_a + alpha (ly - l - y e^{-l}) - ly
    ell[s] = sum_n v_n log p(y_n | l_ns, alpha_s)
    r[n,s] = v_n alpha_s (y_n e^{-l_ns} - 1),   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n alpha_s (c_1 + ly_n - l_ns - y_n e^{-l_ns})

under w ~ N(0, I / prec), alpha ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select.  The prior on the scalar has the negative binomial's form, so the draws, the finish and the
stepper's Adam are tests/_glm_nb_ref.py's by import (log alpha in the place of log phi); the logits come from
tests/_glm_obs_ref.py."""
import math

import numpy as np
from scipy.special import digamma, gammaln

import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

LOG_2PI = nb.LOG_2PI
EPS = 2e-5
_f64 = obs._f64


# ---- inputs shared by tests/test_glm_gamma_cpu.py and tests/test_glm_gamma_gpu.py ----------------------------------------

def make_inputs(B, D, S, seed, mode="both"):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every fifth
    exactly zero) with tau uniform in the accuracy envelope [-2.5, 5] and y drawn from Gamma(shape 2, mean e^{l}) at the
    first draw's logit; every seventh row is scaled by 1000 and every eleventh by 1e-3 (y over six decades about its mean).
    Returns (X, y, W, logshape, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o = mode in ("offset", "both")
    mu = np.exp(obs.logits(X, W, o if use_o else None)[:, 0])
    y = rs.gamma(2.0, mu / 2.0)
    y[6::7] *= 1000.0
    y[3::11] *= 1.0e-3
    y = np.maximum(y, 1.0e-30).astype(np.float32)
    logshape = rs.uniform(-2.5, 5.0, S).astype(np.float32)
    return X, y, W, logshape, (o if use_o else None), (v if mode in ("weights", "both") else None)


# ---- the pass -------------------------------------------------------------------------------------------------------

def shape_constants(alpha):
    """c_a = alpha log alpha - lnGamma(alpha) and c_1 = log alpha + 1 - psi(alpha)."""
    return alpha * np.log(alpha) - gammaln(alpha), np.log(alpha) + 1.0 - digamma(alpha)


def _terms(X, y, W, logshape, offset, weights):
    """Per (row, draw): the terms of ell, their absolute sizes, the residual, the terms of T, their absolute sizes."""
    L = obs.logits(X, W, offset)
    y64 = _f64(y)[:, None]
    alpha = np.exp(_f64(logshape))[None, :]
    c_a, c_1 = shape_constants(alpha)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ly = np.log(y64)
        q = y64 * np.exp(-L)
        x = ly - L
        t_ell = np.where(on, vv * (c_a + alpha * (x - q) - ly), 0.0)
        a_ell = np.where(on, vv * (np.abs(c_a) + alpha * (np.abs(x) + q) + np.abs(ly) + 1.0), 0.0)
        r = np.where(on, vv * alpha * (q - 1.0), 0.0)
        t_T = np.where(on, vv * alpha * (c_1 + x - q), 0.0)
        a_T = np.where(on, vv * (alpha * (np.abs(c_1) + np.abs(x) + q) + 1.0), 0.0)
    return t_ell, a_ell, r, t_T, a_T


def data_pass(X, y, W, logshape, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, t_T, _ = _terms(X, y, W, logshape, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, logshape, offset=None, weights=None):
    """What the device's errors of ell and T are measured against (each times 2e-5), rows of weight 0 left out:
    b_ell = sum_n v (|c_a| + alpha (|ly - l| + y e^{-l}) + |ly| + 1),  b_T = sum_n v (alpha (|c_1| + |ly - l| + y e^{-l}) + 1)."""
    _, a_ell, _, _, a_T = _terms(X, y, W, logshape, offset, weights)
    return a_ell.sum(axis=0), a_T.sum(axis=0)


def row_logpdf(L, y, logshape):
    """log p(y_n | l_ns, alpha_s), the full density: [B, S]."""
    y64 = _f64(y)[:, None]
    alpha = np.exp(_f64(logshape))[None, :]
    c_a, _ = shape_constants(alpha)
    ly = np.log(y64)
    return c_a + alpha * (ly - L - y64 * np.exp(-L)) - ly


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def data_pass_f32(X, y, W, logshape, offset=None, weights=None):
    """The same formulas evaluated plainly in float32, row after row; the two per-draw constants are float64 values
    rounded, as on the device.  The sums follow the pass's design, float32 partials finished in float64: F32_BLOCK rows
    are added one after the other in float32 (the largest partial of a pass that runs one tile per wave, which every
    batch of the parity tests does), the partials in float64.  One float32 sum over all rows would measure its own
    length, not the formulas: over 1003 rows it reaches 1.1e-6 of b_ell where the terms alone are at 1e-7."""
    f = np.float32
    B = np.shape(X)[0]
    if B > F32_BLOCK:
        cut = lambda a, k: None if a is None else a[k:k + F32_BLOCK]
        parts = [data_pass_f32(X[k:k + F32_BLOCK], y[k:k + F32_BLOCK], W, logshape, cut(offset, k), cut(weights, k))
                 for k in range(0, B, F32_BLOCK)]
        return tuple(np.sum([p[i].astype(np.float64) for p in parts], axis=0) for i in range(3))
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, logshape))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    alpha = np.exp(tau).astype(f)
    c_a, c_1 = (c.astype(f) for c in shape_constants(alpha.astype(np.float64)))
    ell, G, T = np.zeros(S, f), np.zeros((S, D), f), np.zeros(S, f)
    one = f(1.0)
    for n in range(B):
        if not v[n] > 0:
            continue
        l = ((X[n][None, :] * W).sum(axis=1, dtype=f) + o[n]).astype(f)
        ly = np.log(y[n]).astype(f)
        q = (y[n] * np.exp(-l).astype(f)).astype(f)
        d = ((ly - l).astype(f) - q).astype(f)
        ell += (v[n] * ((c_a + alpha * d).astype(f) - ly)).astype(f)
        T += (v[n] * (alpha * (c_1 + d).astype(f))).astype(f)
        G += (v[n] * (alpha * (q - one)))[:, None] * X[n][None, :]
    return ell, G, T


# ---- draws and the finish: the negative binomial's (the scalar's prior has the same form) ---------------------------------

init_lam = nb.init_lam              # m = 0 (tau = 0), rho = log 0.1
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1]
draw = nb.draw                      # (W [S, D] float32, logshape [S] float32)
log_prior_tau = nb.log_prior_tau
elbo_and_grad = nb.elbo_and_grad    # (lam, eps, W, logshape, ell, G, T, scale, prec, a0, b0)
update = nb.finish                  # bsc_glm_gamma_update from given statistics: (lam', m1', m2', elbo, grad)


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as GammaReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logshape = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, logshape, offset, weights)
    return update(lam, m1, m2, t, eps, W, logshape, ell, G, T, n_total / B, prec, a0, b0, lr)


def elbo_terms_size(W, logshape, ell_bound, scale, prec=1.0, a0=1.0, b0=1.0, rho=None):
    """The sum of the absolute values of the ELBO's terms, from reference quantities alone: mean_s [scale b_ell_s +
    prec / 2 |w_s|^2 + |a0 tau_s| + b0 alpha_s] + |constants| + sum |rho| + P / 2 (1 + log 2 pi)."""
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


def predict(X, W, logshape, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    alpha = np.exp(_f64(logshape))[None, :]
    mu = np.exp(L)
    v = mu * mu / alpha
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        lp = row_logpdf(L, y, logshape)
        m = lp.max(axis=1, keepdims=True)
        out["lpd"] = m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, W, logshape, y=None, offset=None, weights=None):
    """tests/_glm_nb_ref.predict_bounds' construction for this family.  With a_ns = sum_d |x_nd w_sd| + |o_n| the size of
    the logit's float32 terms and EPS = 2e-5:  mu = exp(l), mu' = mu: e_mu = EPS (mu a + mu), the Poisson family's;
    v = mu^2 / alpha, dv/dl = 2 v: e_v = EPS (2 v a + v), the second term also covering the float32 alpha;  log p: EPS
    times the sizes of its terms, |c_a| + alpha (|ly - l| + y e^{-l}) + |ly| + 1 (the pass's ell bound per row), maximum
    over the draws.  (The logit's own error enters log p through alpha (y e^{-l} - 1), which alpha (|ly - l| + y e^{-l})
    covers: e^x + |x| >= 1 for every x.)"""
    X64, W64 = _f64(X), _f64(W)
    L = obs.logits(X, W, offset)
    a = np.abs(X64) @ np.abs(W64).T
    if offset is not None:
        a = a + np.abs(_f64(offset))[:, None]
    alpha = np.exp(_f64(logshape))[None, :]
    mu = np.exp(L)
    v = mu * mu / alpha
    e_mu = EPS * (mu * a + mu)
    e_v = EPS * (2.0 * v * a + v)
    mean = mu.mean(axis=1)
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = _f64(y)[:, None]
        c_a, _ = shape_constants(alpha)
        ly = np.log(y64)
        e = EPS * (np.abs(c_a) + alpha * (np.abs(ly - L) + y64 * np.exp(-L)) + np.abs(ly) + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
