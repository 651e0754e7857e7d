"""Float64 numpy restatement of the Student-t route (include/bayesic_hip.h: bsc_glm_studentt_data_pass,
bsc_glm_studentt_update, bsc_studentt_predict_pass; svi/glm_studentt.py):

    y_n ~ StudentT(df = nu, location l, scale sigma),  l[n,s] = x_n . w_s + o_n,  k_s = 1 / sigma_s = e^{tau_s}
    z = k (y - l),   u = z^2,   c_nu = lnGamma((nu + 1) / 2) - lnGamma(nu / 2) - log(nu pi) / 2
    log p  = tau + c_nu - ((nu + 1) / 2) log1p(u / nu)
    ell[s] = sum_n v_n log p
    r[n,s] = v_n k_s (nu + 1) z / (nu + u),   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n nu (1 - u) / (nu + u)

under w ~ N(0, I / prec), k ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0 are
dropped by a select, whatever they hold.  The prior on e^tau has the negative binomial's form, so the draws, the finish
and the stepper's Adam are tests/_glm_nb_ref.py's by import (log(1 / sigma) in the place of log phi); the logits come
from tests/_glm_obs_ref.py.  lnGamma is scipy's gammaln.

The bound quantities (``bounds``, ``predict_bounds``) are tests/_glm_lognormal_ref.py's construction: the sums of the
absolute sizes of the terms, with the conditioning of z on its rounded inputs.  z = k (y - l) is formed in float32 from a
rounded k, a rounded y and a logit whose float32 terms have the size a = sum_d |x_d w_d| + |o|, so its absolute error is
a multiple of eps times c = |z| + k (|y| + a).  With g(z) = (nu + 1) z / (nu + u), the derivative of log p in l over k
(and minus its derivative in z), and h(z) = nu (1 - u) / (nu + u):
    g'(z) = (nu + 1)(nu - u) / (nu + u)^2,        h'(z) = -2 nu (nu + 1) z / (nu + u)^2
Per kept (row, draw), times the weight:
    ell:  |tau| + |c_nu| + ((nu + 1) / 2) log1p(u / nu) + |g| c + 1
    r:    k ( |g| + |g'| c )
    T:    |h| + |h'| c + 1
A device result is held to EPS = 2e-5 times these (EPS is tests/_glm_lognormal_ref.py's), a plain float32 replay of the
device's forms to 1e-6 times these (tests/test_glm_studentt_cpu.py)."""
import math

import numpy as np
from scipy.special import gammaln

import _glm_lognormal_ref as lognormal
import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

EPS = lognormal.EPS              # 2e-5
TAU_LO, TAU_HI = -3.0, 5.0       # the range of tau the tests cover (sigma from 20 down to 0.0067)
NUS = (1.0, 2.5, 4.0, 30.0, 1.0e6)      # every one exact in float32
Z_LO, Z_HI = 1.0e-3, 1.0e4       # the designed |z| at the first draw: log-uniform, gross outliers included
DEAD_Y = (np.nan, np.inf, -np.inf, 0.0)         # what the rows of weight 0 hold, in turn
_f64 = obs._f64
logit_size = lognormal.logit_size


def log_norm(nu):
    """c_nu in float64."""
    nu = float(nu)
    return float(gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu) - 0.5 * math.log(nu * math.pi))


# ---- inputs shared by tests/test_glm_studentt_cpu.py and tests/test_glm_studentt_gpu.py ---------------------------------

def make_inputs(B, D, S, seed, mode="both", tau=None, unit=1.0):
    """tests/_glm_lognormal_ref.make_inputs' recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with
    every fifth exactly zero) with tau spread over [-3, 5] (``tau``: given) and responses y_n = l_n0 +- zeta_n / k_0 at the
    FIRST draw's logit and scale, zeta_n log-uniform over [1e-3, 1e4]: the first draw sees every size of residual from a
    row on the fit to a gross outlier, the other draws see the same rows through their own logits and scales (|z| up to
    k_max / k_min times as large; every term stays finite while z^2 does).  nu is not an input of the data: the same
    batch is passed at every nu.  The first column of X is 1 (an intercept) and 70 % of the rows lie above their location,
    so that column's gradient does not cancel.  ``unit``: the size of the logits -- W and the offsets are multiplied by
    it; with unit = 1 / k the data have the size of the noise, with unit = 1 and k = e^5 they are hundreds of sigma
    away from 0, which is the harder case for float32 (z = k (y - l) cancels) and the one the parity tests run.  With
    weights, the rows of weight 0 hold NaN, +inf, -inf and 0 in turn.
    Returns (X, y, W, loginvscale, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    X[:, 0] = 1.0
    W = (0.6 * unit * rs.standard_normal((S, D))).astype(np.float32)
    o = (unit * rs.standard_normal(B)).astype(np.float32)
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
    L0 = obs.logits(X, W, o if use_o else None)[:, 0]
    zeta = np.exp(rs.uniform(math.log(Z_LO), math.log(Z_HI), B))
    zeta[:2] = Z_LO, Z_HI                                   # both ends are there
    sign = np.where(rs.uniform(size=B) < 0.3, -1.0, 1.0)
    y = (L0 + sign * zeta / math.exp(float(lis[0]))).astype(np.float32)
    if use_v:
        dead = np.flatnonzero(v == 0)
        for i, bad in enumerate(DEAD_Y):
            y[dead[i::len(DEAD_Y)]] = bad
    return X, y, W, lis, (o if use_o else None), (v if use_v else None)


# ---- the pass -------------------------------------------------------------------------------------------------------

def _terms(X, y, W, loginvscale, nu, offset, weights):
    """Per (row, draw): the terms of ell, the residual, the terms of T, and the three bound quantities."""
    nu = float(nu)
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    y64 = _f64(y)[:, None]
    tau = _f64(loginvscale)[None, :]
    k = np.exp(tau)
    cn = log_norm(nu)
    hn = 0.5 * (nu + 1.0)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        z = k * (y64 - L)
        az = np.abs(z)
        u = z * z
        lp = np.log1p(u / nu)
        den = nu + u
        g = (nu + 1.0) * z / den
        dg = (nu + 1.0) * np.abs(nu - u) / (den * den)
        h = nu * (1.0 - u) / den
        dh = 2.0 * nu * (nu + 1.0) * az / (den * den)
        c = az + k * (np.abs(y64) + a)
        t_ell = np.where(on, vv * (tau + cn - hn * lp), 0.0)
        a_ell = np.where(on, vv * (np.abs(tau) + abs(cn) + hn * lp + np.abs(g) * c + 1.0), 0.0)
        r = np.where(on, vv * k * g, 0.0)
        a_r = np.where(on, vv * k * (np.abs(g) + dg * c), 0.0)
        t_T = np.where(on, vv * h, 0.0)
        a_T = np.where(on, vv * (np.abs(h) + dh * c + 1.0), 0.0)
    return t_ell, a_ell, r, a_r, t_T, a_T


def data_pass(X, y, W, loginvscale, nu, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, _, t_T, _ = _terms(X, y, W, loginvscale, nu, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, loginvscale, nu, offset=None, weights=None):
    """(b_ell [S], b_G [S, D], b_T [S]): what the errors are measured against (module docstring), rows of weight 0 left
    out; b_G[s,d] = sum_n a_r[n,s] |x_nd|."""
    _, a_ell, _, a_r, _, a_T = _terms(X, y, W, loginvscale, nu, offset, weights)
    return a_ell.sum(axis=0), a_r.T @ np.abs(_f64(X)), a_T.sum(axis=0)


def row_logpdf(L, y, loginvscale, nu):
    """log p(y | l, k) per (row, draw): [B, S]."""
    nu = float(nu)
    tau = _f64(loginvscale)[None, :]
    z = np.exp(tau) * (_f64(y)[:, None] - L)
    return tau + log_norm(nu) - 0.5 * (nu + 1.0) * np.log1p(z * z / nu)


def gaussian_pass(X, y, W, loginvscale, offset=None, weights=None):
    """The limit nu -> infinity: log p = tau - log(2 pi) / 2 - z^2 / 2, d / d l = k z, d / d tau = 1 - z^2."""
    L = obs.logits(X, W, offset)
    tau = _f64(loginvscale)[None, :]
    k = np.exp(tau)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    keep = v > 0
    vv = v[keep][:, None]
    z = k * (_f64(y)[keep][:, None] - L[keep])
    ell = (vv * (tau - 0.5 * nb.LOG_2PI - 0.5 * z * z)).sum(axis=0)
    G = (vv * k * z).T @ _f64(X)[keep]
    T = (vv * (1.0 - z * z)).sum(axis=0)
    return ell, G, T


# ---- the device's forms in plain float32 ----------------------------------------------------------------------------------

_fma = lognormal._fma
F32_BLOCK = lognormal.F32_BLOCK


def link_f32(l, y, v, tau, nu):
    """csrc/bsc_families.h's StudentT::glm_link step by step on float32 arrays: l [B, S] the logits, y and v [B], tau [S].
    Returns the terms of ell, the residuals and the terms of T, each [B, S] float32.  The per-launch constants are made
    as StudentT::glm_disp makes them: k = expf(tau), tau + c_nu in float64 rounded once; 1 / nu is a correctly rounded
    division and the hardware reciprocal of nu + z^2 is 1 / x rounded to float32."""
    f = np.float32
    one, zero = f(1.0), f(0.0)
    nu = f(nu)
    l, y, v, tau = (np.asarray(a, f) for a in (l, y, v, tau))
    k = np.exp(tau)[None, :]
    lg = (_f64(tau) + log_norm(float(nu))).astype(f)[None, :]
    np1 = nu + one
    inu = one / nu
    keep = v > 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # every array below is float32
        vq = np.where(keep, v, zero)[:, None]               # the selects sit on the inputs, as in the link
        yq = np.where(keep, y, zero)[:, None]
        lq = np.where(keep[:, None], l, zero)
        z = k * (yq - lq)
        zz = z * z
        r = zz * inu
        t = one + r
        tiny = t == one
        lp = np.log(t) * (r / np.where(tiny, one, t - one)) + np.where(tiny, r, zero)
        q = one / _fma(z, z, np.full_like(z, nu))
        t_ell = vq * _fma(np.full_like(lp, f(-0.5) * np1), lp, np.broadcast_to(lg, lp.shape))
        t_T = vq * ((nu * (one - zz)) * q)
        res = vq * ((k * np1) * (z * q))
    assert t_ell.dtype == f and t_T.dtype == f and res.dtype == f and z.dtype == f
    return t_ell, res, t_T


def data_pass_f32(X, y, W, loginvscale, nu, offset=None, weights=None):
    """link_f32 on the logits of one float32 matrix product, float32 partials of F32_BLOCK rows finished in float64
    (tests/_glm_lognormal_ref.data_pass_f32)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, loginvscale))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    with np.errstate(over="ignore", invalid="ignore"):
        l = X @ W.T + o[:, None]
    assert l.dtype == f
    t_ell, r, t_T = link_f32(l, y, v, tau, nu)
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
update = nb.finish                  # bsc_glm_studentt_update from given statistics: (lam', m1', m2', elbo, grad)
elbo_terms_size = lognormal.elbo_terms_size


def step(lam, m1, m2, t, X, y, nu, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as StudentTReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, lis = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, lis, nu, offset, weights)
    return update(lam, m1, m2, t, eps, W, lis, ell, G, T, n_total / B, prec, a0, b0, lr)


def fit(X, y, nu, S, seed, steps, lr, prec=1.0, a0=1.0, b0=0.1, offset=None, weights=None, n_total=None):
    """The reference driver: ``steps`` full-batch updates from init_lam; returns lam."""
    lam = init_lam(X.shape[1])
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    n_total = float(X.shape[0]) if n_total is None else n_total
    for t in range(1, steps + 1):
        lam, m1, m2, _, _ = step(lam, m1, m2, t, X, y, nu, S, seed, n_total, lr, prec, a0, b0, offset, weights)
    return lam


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], loginvscale float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def variance(tau, nu):
    """nu / ((nu - 2) k^2) for nu > 2, +inf otherwise."""
    k2 = np.exp(2.0 * np.asarray(tau, np.float64))
    return nu / ((nu - 2.0) * k2) if nu > 2.0 else np.full_like(k2, np.inf)


_lse_mean = lognormal._lse_mean


def predict(X, W, loginvscale, nu, y=None, offset=None, weights=None):
    """mean (of the location), var (law of total variance, centred; +inf for nu <= 2) and, with y, lpd and lpd_sum
    (weighted with weights)."""
    L = obs.logits(X, W, offset)
    v = np.broadcast_to(variance(_f64(loginvscale)[None, :], float(nu)), L.shape)
    mean = L.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((L - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = _lse_mean(row_logpdf(L, y, loginvscale, nu))
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, W, loginvscale, nu, y=None, offset=None, weights=None):
    """tests/_glm_lognormal_ref.predict_bounds' construction for this family.  With a = logit_size and EPS = 2e-5:
    mu = l, whose float32 terms have the size a: e_mu = EPS a;  v = nu / ((nu - 2) k^2), one rounded constant per draw:
    e_v = EPS v (nu <= 2: the device's +inf is compared exactly, the bound is 0);  log p: EPS times the pass's per-row
    ell quantity (module docstring), maximum over the draws."""
    nu = float(nu)
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    tau = _f64(loginvscale)[None, :]
    k = np.exp(tau)
    e_mu = EPS * a
    mean = L.mean(axis=1)
    dev = np.abs(L - mean[:, None])
    e_v = EPS * variance(tau, nu) if nu > 2.0 else np.zeros_like(tau)
    out = dict(mean=e_mu.mean(axis=1),
               var=np.broadcast_to(e_v, L.shape).mean(axis=1)
               + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((L - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = _f64(y)[:, None]
        z = k * (y64 - L)
        az = np.abs(z)
        u = z * z
        c = az + k * (np.abs(y64) + a)
        g = (nu + 1.0) * az / (nu + u)
        e = EPS * (np.abs(tau) + abs(log_norm(nu)) + 0.5 * (nu + 1.0) * np.log1p(u / nu) + g * c + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
