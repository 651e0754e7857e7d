"""Float64 numpy restatement of the GLM path (include/bayesic_hip.h: bsc_glm_data_pass, bsc_glm_update;
svi/glm.py): Bernoulli-logit and Poisson-log regression under w ~ N(0, I / tau), mean-field Gaussian guide
lam = [m (D) | rho (D)].  Draws and Adam come from the oracle by import (Philox stream 0, as oracle.svi.blr_sample)."""
import math

import numpy as np

from oracle import philox, svi

LOG_2PI = math.log(2.0 * math.pi)


def log_partition(link, L):
    """A(l) and A'(l): softplus / sigmoid (logistic), exp / exp (poisson), float64."""
    if link == "logistic":
        e = np.exp(-np.abs(L))
        return np.maximum(L, 0.0) + np.log1p(e), np.where(L >= 0.0, 1.0, e) / (1.0 + e)
    if link == "poisson":
        e = np.exp(L)
        return e, e
    raise ValueError(link)


def glm_data_pass(link, X, y, W):
    """ell[s] = sum_n [y_n l_ns - A(l_ns)], G[s, :] = sum_n (y_n - A'(l_ns)) x_n with l = X W^T: float32 operands,
    float64 arithmetic.  Returns (ell [S], G [S, D])."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    y64 = np.asarray(y, np.float32).astype(np.float64)
    W64 = np.asarray(W, np.float32).astype(np.float64)
    L = X64 @ W64.T
    A, dA = log_partition(link, L)
    return (y64[:, None] * L - A).sum(axis=0), (y64[:, None] - dA).T @ X64


def init_lam(D):
    """The driver's default: m = 0, rho = log 0.1."""
    lam = np.zeros(2 * D)
    lam[D:] = math.log(0.1)
    return lam


def noise(D, S, seed, step):
    return philox.normal_draws(seed, S, D, stream=0, step=step)


def draw(lam, eps):
    """w_s = m + e^rho eps_s rounded to float32 (what the pass reads and the prior term sees)."""
    D = eps.shape[1]
    lam = np.asarray(lam, np.float64)
    return (lam[None, :D] + np.exp(lam[D:])[None, :] * eps).astype(np.float32)


def glm_elbo_and_grad(lam, eps, W, ell, G, scale, tau):
    """elbo = mean_s [scale ell_s - tau/2 |w_s|^2] + D/2 log(tau / 2 pi) + sum rho + D/2 (1 + log 2 pi);
    g_s = scale G_s - tau w_s;  d/d m = mean_s g_s,  d/d rho = mean_s g_s eps_s e^rho + 1."""
    lam = np.asarray(lam, np.float64)
    S, D = W.shape
    rho = lam[D:]
    W64 = np.asarray(W, np.float64)
    f = scale * ell - 0.5 * tau * (W64 * W64).sum(axis=1)
    elbo = f.mean() + 0.5 * D * math.log(tau / (2.0 * math.pi)) + rho.sum() + 0.5 * D * (1.0 + LOG_2PI)
    g = scale * G - tau * W64
    return elbo, np.concatenate([g.mean(axis=0), (g * eps).mean(axis=0) * np.exp(rho) + 1.0])


def finish(lam, m1, m2, t, eps, W, ell, G, scale, tau, lr):
    """bsc_glm_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = glm_elbo_and_grad(lam, eps, W, ell, G, scale, tau)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr)
    return lam2, m1, m2, elbo, grad


def glm_step(link, lam, m1, m2, t, X, y, S, seed, n_total, lr, tau=1.0):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as GLMReparamSVI does it.
    Returns (lam, m1, m2, elbo, grad)."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W = draw(lam, eps)
    ell, G = glm_data_pass(link, X, y, W)
    return finish(lam, m1, m2, t, eps, W, ell, G, n_total / B, tau, lr)


def elbo_fixed_draws(link, lam, eps, X, y, scale, tau):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of
    the draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    D = eps.shape[1]
    W = lam[None, :D] + np.exp(lam[D:])[None, :] * eps
    L = np.asarray(X, np.float64) @ W.T
    A, _ = log_partition(link, L)
    ell = (np.asarray(y, np.float64)[:, None] * L - A).sum(axis=0)
    f = scale * ell - 0.5 * tau * (W * W).sum(axis=1)
    return f.mean() + 0.5 * D * math.log(tau / (2.0 * math.pi)) + lam[D:].sum() + 0.5 * D * (1.0 + LOG_2PI)
