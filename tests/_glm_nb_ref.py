"""Float64 numpy restatement of the negative-binomial route (include/bayesic_hip.h: bsc_glm_nb_data_pass,
bsc_glm_nb_update, bsc_nb_predict_pass; svi/glm_nb.py):

    y_n ~ NegBin(mean exp(l_n), dispersion phi),  l[n,s] = x_n . w_s + o_n,  u = l - tau_s,  phi_s = e^{tau_s}
    ell[s] = sum_n v_n [ dlnGamma(y_n, phi_s) + y_n u - (y_n + phi_s) softplus(u) ]
    r[n,s] = v_n [ y_n - (y_n + phi_s) sigmoid(u) ],   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n [ phi_s dpsi(y_n, phi_s) - phi_s softplus(u) ] - sum_n r[n,s]

under w ~ N(0, I / prec), phi ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select.  The logistic forms, Adam and the draws come from tests/_glm_ref.py / tests/_glm_obs_ref.py and
the oracle by import."""
import math

import numpy as np
from scipy.special import digamma, gammaln

import _glm_obs_ref as obs
import _glm_ref as glm
from oracle import philox, svi

LOG_2PI = glm.LOG_2PI
EPS = 2e-5
_f64 = obs._f64


# ---- inputs shared by tests/test_glm_nb_cpu.py and tests/test_glm_nb_gpu.py ----------------------------------------------

def make_inputs(B, D, S, seed, mode="both"):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every fifth
    exactly zero) with tau uniform in the accuracy envelope [-2.5, 5] and NB(phi = 2, mean 1.5) counts (about a third
    of them 0), every seventh replaced by a draw from [100, 3000).
    Returns (X, y, W, logphi, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    y = rs.negative_binomial(2, 2.0 / 3.5, size=B).astype(np.float32)
    big = rs.randint(100, 3000, size=B).astype(np.float32)
    y[6::7] = big[6::7]
    logphi = rs.uniform(-2.5, 5.0, S).astype(np.float32)
    return X, y, W, logphi, (o if mode in ("offset", "both") else None), (v if mode in ("weights", "both") else None)


# ---- the pass -------------------------------------------------------------------------------------------------------

def _terms(X, y, W, logphi, offset, weights):
    """Per (row, draw): the terms of ell, their absolute sizes, the residual, the terms of T, their absolute sizes."""
    L = obs.logits(X, W, offset)
    y64 = _f64(y)[:, None]
    tau = _f64(logphi)[None, :]
    phi = np.exp(tau)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        u = L - tau
        sp, sg = glm.log_partition("logistic", u)
        pos = y64 > 0.0
        dlg = np.where(pos, gammaln(y64 + phi) - gammaln(phi), 0.0)
        dps = np.where(pos, digamma(y64 + phi) - digamma(phi), 0.0)
        res = y64 - (y64 + phi) * sg
        t_ell = np.where(on, vv * (dlg + y64 * u - (y64 + phi) * sp), 0.0)
        a_ell = np.where(on, vv * (np.abs(dlg) + np.abs(y64 * u) + (y64 + phi) * sp + 1.0), 0.0)
        r = np.where(on, vv * res, 0.0)
        t_T = np.where(on, vv * (phi * dps - phi * sp) - vv * res, 0.0)
        a_T = np.where(on, vv * (phi * np.abs(dps) + phi * sp + np.abs(res) + 1.0), 0.0)
    return t_ell, a_ell, r, t_T, a_T


def data_pass(X, y, W, logphi, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, t_T, _ = _terms(X, y, W, logphi, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, logphi, offset=None, weights=None):
    """What the device's errors of ell and T are measured against (each times 2e-5), rows of weight 0 left out:
    sum_n v_n (|dlnGamma| + |y u| + (y + phi) sp(u) + 1)   and   sum_n v_n (phi |dpsi| + phi sp(u) + |y - (y + phi) sg(u)| + 1)."""
    _, a_ell, _, _, a_T = _terms(X, y, W, logphi, offset, weights)
    return a_ell.sum(axis=0), a_T.sum(axis=0)


def row_logpmf(L, y, logphi):
    """log p(y_n | l_ns, phi_s), the constant -lnGamma(y + 1) included: [B, S]."""
    y64 = _f64(y)[:, None]
    tau = _f64(logphi)[None, :]
    phi = np.exp(tau)
    u = L - tau
    sp, _ = glm.log_partition("logistic", u)
    return gammaln(y64 + phi) - gammaln(phi) - gammaln(y64 + 1.0) + y64 * u - (y64 + phi) * sp


def _lgamma_digamma_f32(z):
    """The naive float32 evaluation: 8-step recurrence up to z >= 8, three asymptotic terms."""
    f = np.float32
    z = np.asarray(z, f).copy()
    P, dP = np.ones_like(z), np.zeros_like(z)
    for _ in range(8):
        lo = z < f(8)
        dP = np.where(lo, dP * z + P, dP).astype(f)
        P = np.where(lo, P * z, P).astype(f)
        z = np.where(lo, z + f(1), z).astype(f)
    lz = np.log(z).astype(f)
    inv = (f(1) / z).astype(f)
    inv2 = (inv * inv).astype(f)
    lg = ((z - f(0.5)) * lz - z + f(0.9189385332) + inv * (f(1 / 12) - inv2 * (f(1 / 360) - inv2 * f(1 / 1260)))
          - np.log(P).astype(f)).astype(f)
    psi = (lz - f(0.5) * inv - inv2 * (f(1 / 12) - inv2 * (f(1 / 120) - inv2 * f(1 / 252))) - dP / P).astype(f)
    return lg, psi


def data_pass_f32(X, y, W, logphi, offset=None, weights=None):
    """The same formulas evaluated naively in float32, row after row (what a device pass may do at worst)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, logphi))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    phi = np.exp(tau).astype(f)
    lg0, ps0 = _lgamma_digamma_f32(phi)
    ell, G, T = np.zeros(S, f), np.zeros((S, D), f), np.zeros(S, f)
    one = f(1.0)
    for n in range(B):
        if not v[n] > 0:
            continue
        u = ((X[n][None, :] * W).sum(axis=1, dtype=f) + o[n] - tau).astype(f)
        e = np.exp(-np.abs(u)).astype(f)
        sp = (np.maximum(u, f(0)) + np.log1p(e)).astype(f)
        sg = (np.where(u >= 0, one, e) / (one + e)).astype(f)
        z = (y[n] + phi).astype(f)
        if y[n] > 0:
            lg, ps = _lgamma_digamma_f32(z)
            dlg, dps = (lg - lg0).astype(f), (ps - ps0).astype(f)
        else:
            dlg = dps = np.zeros(S, f)
        res = (y[n] - z * sg).astype(f)
        ell += v[n] * (dlg + y[n] * u - z * sp)
        T += v[n] * (phi * (dps - sp) - res)
        G += (v[n] * res)[:, None] * X[n][None, :]
    return ell, G, T


# ---- draws ----------------------------------------------------------------------------------------------------------

def init_lam(D):
    """The driver's default: m = 0 (tau = 0), rho = log 0.1."""
    P = D + 1
    lam = np.zeros(2 * P)
    lam[P:] = math.log(0.1)
    return lam


def noise(D, S, seed, step):
    """bsc_blr_noise(D): [S, D + 1], Philox stream 0 in the columns of w, stream 1 in tau's."""
    return np.concatenate([philox.normal_draws(seed, S, D, stream=0, step=step),
                           philox.normal_draws(seed, S, 1, stream=1, step=step)], axis=1)


def draw(lam, eps):
    """(W [S, D] float32, logphi [S] float32): what the pass reads and the finish uses."""
    P = eps.shape[1]
    lam = np.asarray(lam, np.float64)
    z = (lam[None, :P] + np.exp(lam[P:])[None, :] * eps).astype(np.float32)
    return z[:, :P - 1], z[:, P - 1]


# ---- the finish -----------------------------------------------------------------------------------------------------

def log_prior_tau(tau, a0, b0):
    return a0 * math.log(b0) - math.lgamma(a0) + a0 * tau - b0 * np.exp(tau)


def elbo_and_grad(lam, eps, W, logphi, ell, G, T, scale, prec=1.0, a0=1.0, b0=1.0):
    lam = np.asarray(lam, np.float64)
    S, D = W.shape
    P = D + 1
    rho = lam[P:]
    w, tau = np.asarray(W, np.float64), np.asarray(logphi, np.float64)
    f = scale * ell - 0.5 * prec * (w * w).sum(axis=1) + log_prior_tau(tau, a0, b0)
    elbo = f.mean() + 0.5 * D * math.log(prec / (2.0 * math.pi)) + rho.sum() + 0.5 * P * (1.0 + LOG_2PI)
    g = np.concatenate([scale * G - prec * w, (scale * T + a0 - b0 * np.exp(tau))[:, None]], axis=1)
    return elbo, np.concatenate([g.mean(axis=0), (g * eps).mean(axis=0) * np.exp(rho) + 1.0])


def finish(lam, m1, m2, t, eps, W, logphi, ell, G, T, scale, prec, a0, b0, lr):
    """bsc_glm_nb_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = elbo_and_grad(lam, eps, W, logphi, ell, G, T, scale, prec, a0, b0)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr)
    return lam2, m1, m2, elbo, grad


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as NegBinReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logphi = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, logphi, offset, weights)
    return finish(lam, m1, m2, t, eps, W, logphi, ell, G, T, n_total / B, prec, a0, b0, lr)


def elbo_fixed_draws(lam, eps, X, y, scale, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of
    the draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    P = eps.shape[1]
    D = P - 1
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    w, tau = z[:, :D], z[:, D]
    L = np.asarray(X, np.float64) @ w.T
    if offset is not None:
        L = L + np.asarray(offset, np.float64)[:, None]
    y64 = np.asarray(y, np.float64)[:, None]
    v = np.ones(L.shape[0]) if weights is None else np.asarray(weights, np.float64)
    phi = np.exp(tau)[None, :]
    u = L - tau[None, :]
    sp, _ = glm.log_partition("logistic", u)
    ell = (v[:, None] * (gammaln(y64 + phi) - gammaln(phi) + y64 * u - (y64 + phi) * sp)).sum(axis=0)
    f = scale * ell - 0.5 * prec * (w * w).sum(axis=1) + log_prior_tau(tau, a0, b0)
    return f.mean() + 0.5 * D * math.log(prec / (2.0 * math.pi)) + lam[P:].sum() + 0.5 * P * (1.0 + LOG_2PI)


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], logphi float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def predict(X, W, logphi, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    phi = np.exp(_f64(logphi))[None, :]
    mu = np.exp(L)
    v = mu + mu * mu / phi
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        lp = row_logpmf(L, y, logphi)
        m = lp.max(axis=1, keepdims=True)
        out["lpd"] = m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, W, logphi, y=None, offset=None, weights=None):
    """tests/_predict_ref.bounds' construction for this family.  With a_ns = sum_d |x_nd w_sd| + |o_n| the size of the
    logit's float32 terms and EPS = 2e-5:  mu = exp(l), mu' = mu: e_mu = EPS (mu a + mu), the Poisson family's;
    v = mu + mu^2 / phi, dv/dl = mu + 2 mu^2 / phi: e_v = EPS ((mu + 2 mu^2 / phi) a + v), the second term also covering
    the float32 phi;  log p: EPS times the sizes of its terms, |dlnGamma| + |y u| + (y + phi) sp(u) + lnGamma(y + 1) + 1
    (the pass's ell bound plus the row constant), maximum over the draws."""
    X64, W64 = _f64(X), _f64(W)
    L = obs.logits(X, W, offset)
    a = np.abs(X64) @ np.abs(W64).T
    if offset is not None:
        a = a + np.abs(_f64(offset))[:, None]
    tau = _f64(logphi)[None, :]
    phi = np.exp(tau)
    mu = np.exp(L)
    v = mu + mu * mu / phi
    e_mu = EPS * (mu * a + mu)
    e_v = EPS * ((mu + 2.0 * mu * mu / phi) * a + v)
    mean = mu.mean(axis=1)
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = _f64(y)[:, None]
        u = L - tau
        sp, _ = glm.log_partition("logistic", u)
        dlg = np.where(y64 > 0, gammaln(y64 + phi) - gammaln(phi), 0.0)
        e = EPS * (np.abs(dlg) + np.abs(y64 * u) + (y64 + phi) * sp + gammaln(y64 + 1.0) + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
