"""Float64 numpy restatement of the random-intercept GLM route (include/bayesic_hip.h: bsc_glm_data_pass_groups,
bsc_glm_hier_update; svi/hier_glm.py):

    l[n,s] = x_n . w_s + b_s[g_n] + o_n
    ell[s] = sum_n v_n (y_n l_ns - A(l_ns)),   G[s,:] = sum_n r_ns x_n,   H[s,j] = sum_{n : g_n = j} r_ns,
    r_ns = v_n (y_n - A'(l_ns)),  rows of weight 0 dropped by a select

under w ~ N(0, I / tau_w), b_j | zeta ~ N(0, e^{-zeta}), e^zeta ~ Gamma(a0, b0); z = [w (D) | b (J) | zeta],
lam = [m (P) | rho (P)].  The link functions, Adam and the draws come from tests/_glm_ref.py / tests/_glm_obs_ref.py by
import, the log-prior from oracle.svi.bbvi_log_prior (tau_w = 1; another tau_w changes w's Gaussian alone)."""
import math

import numpy as np

import _glm_obs_ref as obs
import _glm_ref as glm
from oracle import philox, svi

LOG_2PI = glm.LOG_2PI
_f64 = obs._f64


# ---- the pass -------------------------------------------------------------------------------------------------------

def logits(X, g, W, Bm, offset=None):
    """[B, S]; Bm [S, J] are the intercept draws."""
    L = _f64(X) @ _f64(W).T + _f64(Bm)[:, np.asarray(g)].T
    return L if offset is None else L + _f64(offset)[:, None]


def onehot(g, J):
    out = np.zeros((len(g), J), np.float32)
    out[np.arange(len(g)), np.asarray(g)] = 1.0
    return out


def _terms(link, X, y, g, W, Bm, offset, weights):
    L = logits(X, g, W, Bm, offset)
    y64 = _f64(y)[:, None]
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        A, dA = glm.log_partition(link, L)
        t_ell = np.where(on, v[:, None] * (y64 * L - A), 0.0)
        t_abs = np.where(on, v[:, None] * (np.abs(y64 * L) + A + 1.0), 0.0)
        t_res = np.where(on, v[:, None] * (y64 - dA), 0.0)
    return t_ell, t_abs, t_res


def data_pass(link, X, y, g, J, W, Bm, offset=None, weights=None):
    """(ell [S], G [S, D], H [S, J]): float32 operands, float64 arithmetic."""
    t_ell, _, R = _terms(link, X, y, g, W, Bm, offset, weights)
    H = np.zeros((R.shape[1], J))
    np.add.at(H.T, np.asarray(g), R)
    return t_ell.sum(axis=0), R.T @ _f64(X), H


def ell_bound(link, X, y, g, W, Bm, offset=None, weights=None):
    """What the device's ell error is measured against (tests/_glm_obs_ref.ell_bound with the intercept in l)."""
    return _terms(link, X, y, g, W, Bm, offset, weights)[1].sum(axis=0)


def data_pass_f32(link, X, y, g, J, W, Bm, offset=None, weights=None):
    """The same formulas evaluated naively in float32, row after row (what a device pass may do at worst)."""
    X, y, W, Bm = (np.asarray(a, np.float32) for a in (X, y, W, Bm))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, np.float32) if offset is None else np.asarray(offset, np.float32)
    v = np.ones(B, np.float32) if weights is None else np.asarray(weights, np.float32)
    ell, G, H = np.zeros(S, np.float32), np.zeros((S, D), np.float32), np.zeros((S, J), np.float32)
    one = np.float32(1.0)
    for n in range(B):
        if not v[n] > 0:
            continue
        l = (X[n][None, :] * W).sum(axis=1, dtype=np.float32) + Bm[:, g[n]] + o[n]
        if link == "logistic":
            e = np.exp(-np.abs(l)).astype(np.float32)
            a = (np.maximum(l, np.float32(0)) + np.log1p(e)).astype(np.float32)
            da = (np.where(l >= 0, one, e) / (one + e)).astype(np.float32)
        else:
            a = da = np.exp(l).astype(np.float32)
        r = v[n] * (y[n] - da)
        ell += v[n] * (y[n] * l - a)
        G += r[:, None] * X[n][None, :]
        H[:, g[n]] += r
    return ell, G, H


# ---- draws ----------------------------------------------------------------------------------------------------------

def init_lam(P):
    """The driver's default: m = 0, rho = log 0.1."""
    lam = np.zeros(2 * P)
    lam[P:] = math.log(0.1)
    return lam


def noise(D, J, S, seed, step):
    """bsc_blr_noise(D + J): [S, P], Philox stream 0 in the columns of w and b, stream 1 in zeta's."""
    return np.concatenate([philox.normal_draws(seed, S, D + J, stream=0, step=step),
                           philox.normal_draws(seed, S, 1, stream=1, step=step)], axis=1)


def draw(lam, eps, D, J):
    """(W [S, D] float32, Bm [S, J] float32, zeta [S] float64): what the pass reads, and zeta as the finish forms it."""
    P = D + J + 1
    lam = np.asarray(lam, np.float64)
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    return z[:, :D].astype(np.float32), z[:, D:D + J].astype(np.float32), z[:, P - 1]


def chunked(Bm):
    """[S, J] -> the pass's float32 [ceil(S / 8)][J][8] (chunk, group, draw slot), unused slots zero, flat."""
    S, J = Bm.shape
    out = np.zeros(((S + 7) // 8, J, 8), np.float32)
    for s in range(S):
        out[s // 8, :, s % 8] = Bm[s]
    return out.reshape(-1)


def unchunk(flat, S, J):
    a = np.asarray(flat).reshape(-1, J, 8)
    return np.stack([a[s // 8, :, s % 8] for s in range(S)])


# ---- the finish -----------------------------------------------------------------------------------------------------

def log_prior(w, b, zeta, tau=1.0, a0=1.0, b0=1.0):
    """oracle.svi.bbvi_log_prior with w ~ N(0, I / tau)."""
    D, J = w.shape[1], b.shape[1]
    z = np.concatenate([w, b, zeta[:, None]], axis=1)
    return svi.bbvi_log_prior(z, D, J, a0, b0) + 0.5 * D * math.log(tau) - 0.5 * (tau - 1.0) * (w * w).sum(axis=1)


def elbo_and_grad(lam, eps, W, Bm, zeta, ell, G, H, scale, tau=1.0, a0=1.0, b0=1.0):
    lam = np.asarray(lam, np.float64)
    S, D = W.shape
    J = Bm.shape[1]
    P = D + J + 1
    rho = lam[P:]
    w, b = np.asarray(W, np.float64), np.asarray(Bm, np.float64)
    ez = np.exp(zeta)
    f = scale * ell + log_prior(w, b, zeta, tau, a0, b0)
    elbo = f.mean() + rho.sum() + 0.5 * P * (1.0 + LOG_2PI)
    g = np.concatenate([scale * G - tau * w, scale * H - ez[:, None] * b,
                        (0.5 * J + a0 - ez * (b0 + 0.5 * (b * b).sum(axis=1)))[:, None]], axis=1)
    return elbo, np.concatenate([g.mean(axis=0), (g * eps).mean(axis=0) * np.exp(rho) + 1.0])


def finish(lam, m1, m2, t, eps, W, Bm, zeta, ell, G, H, scale, tau, a0, b0, lr):
    """bsc_glm_hier_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = elbo_and_grad(lam, eps, W, Bm, zeta, ell, G, H, scale, tau, a0, b0)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr)
    return lam2, m1, m2, elbo, grad


def step(link, lam, m1, m2, t, X, y, g, J, S, seed, n_total, lr, tau=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as HierGLMReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, J, S, seed, t - 1)
    W, Bm, zeta = draw(lam, eps, D, J)
    ell, G, H = data_pass(link, X, y, g, J, W, Bm, offset, weights)
    return finish(lam, m1, m2, t, eps, W, Bm, zeta, ell, G, H, n_total / B, tau, a0, b0, lr)


def elbo_fixed_draws(link, lam, eps, X, y, g, J, scale, tau=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of
    the draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    D = X.shape[1]
    P = D + J + 1
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    w, b, zeta = z[:, :D], z[:, D:D + J], z[:, P - 1]
    L = np.asarray(X, np.float64) @ w.T + b[:, np.asarray(g)].T
    if offset is not None:
        L = L + np.asarray(offset, np.float64)[:, None]
    v = np.ones(L.shape[0]) if weights is None else np.asarray(weights, np.float64)
    A, _ = glm.log_partition(link, L)
    ell = (v[:, None] * (np.asarray(y, np.float64)[:, None] * L - A)).sum(axis=0)
    f = scale * ell + log_prior(w, b, zeta, tau, a0, b0)
    return f.mean() + lam[P:].sum() + 0.5 * P * (1.0 + LOG_2PI)
