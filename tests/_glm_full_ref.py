"""Float64 numpy restatement of one update of the full-covariance Gaussian guide of the GLM path
(include/bayesic_hip.h, bsc_glm_fullrank_update; svi/glm.py, covariance="full"): q(w) = N(mu, L L^T) over w in R^D,
L lower-triangular with L_ii = e^{rho_i}, lam = [mu (D) | L packed row-major, lower triangle incl. the diagonal
(D(D+1)/2)], rho_i in the diagonal slots.  The model, the data pass, the noise and Adam are tests/_glm_ref.py's."""
import math

import numpy as np

from oracle import svi

import _glm_ref as mf

LOG_2PI = math.log(2.0 * math.pi)


def n_lam(D):
    return D + D * (D + 1) // 2


def diag_slots(D):
    i = np.arange(D)
    return D + i * (i + 1) // 2 + i


def unpack(lam, D):
    """(mu [D], L [D, D]) with the diagonal exponentiated."""
    lam = np.asarray(lam, np.float64)
    L = np.zeros((D, D))
    L[np.tril_indices(D)] = lam[D:]
    d = np.arange(D)
    L[d, d] = np.exp(L[d, d])
    return lam[:D].copy(), L


def pack(mu, L):
    """Inverse of unpack (L's diagonal must be positive)."""
    D = len(mu)
    Lr = np.array(L, np.float64)
    d = np.arange(D)
    Lr[d, d] = np.log(Lr[d, d])
    return np.concatenate([np.asarray(mu, np.float64), Lr[np.tril_indices(D)]])


def init_lam(D):
    """The driver's default: mu = 0, rho = log 0.1, zero off-diagonal entries."""
    lam = np.zeros(n_lam(D))
    lam[diag_slots(D)] = math.log(0.1)
    return lam


def from_mean_field(lam_mf, D):
    """[m | rho] -> the full layout with zero off-diagonal entries."""
    lam_mf = np.asarray(lam_mf, np.float64)
    lam = np.zeros(n_lam(D))
    lam[:D] = lam_mf[:D]
    lam[diag_slots(D)] = lam_mf[D:]
    return lam


def to_mean_field(v, D):
    """The mu and diagonal entries of a vector in lam's layout, as [m | rho]."""
    v = np.asarray(v, np.float64)
    return np.concatenate([v[:D], v[diag_slots(D)]])


def noise(D, S, seed, step):
    """Columns 0 .. D-1 of bsc_blr_noise's [S, D+1] (Philox stream 0)."""
    return mf.noise(D, S, seed, step)


def draw(lam, eps):
    """w_s = mu + L eps_s rounded to float32 (what the pass reads and the prior term sees)."""
    D = eps.shape[1]
    mu, L = unpack(lam, D)
    return (mu[None, :] + eps @ L.T).astype(np.float32)


def elbo_and_grad(lam, eps, W, ell, G, scale, tau):
    """_glm_ref.glm_elbo_and_grad extended to L: g_s = scale G_s - tau w_s (W as given: the device's are
    float32-rounded), d/d mu = mean_s g_s, d/d L_ij = mean_s g_si eps_sj (j < i), d/d rho_i = mean_s g_si eps_si e^{rho_i} + 1."""
    lam = np.asarray(lam, np.float64)
    S, D = eps.shape
    rho = lam[diag_slots(D)]
    W64 = np.asarray(W, np.float64)
    f = scale * np.asarray(ell, np.float64) - 0.5 * tau * (W64 * W64).sum(axis=1)
    elbo = f.mean() + 0.5 * D * math.log(tau / (2.0 * math.pi)) + rho.sum() + 0.5 * D * (1.0 + LOG_2PI)
    g = scale * np.asarray(G, np.float64) - tau * W64
    gL = (g.T @ eps) / S
    d = np.arange(D)
    gL[d, d] = (g * eps).mean(axis=0) * np.exp(rho) + 1.0
    return elbo, np.concatenate([g.mean(axis=0), gL[np.tril_indices(D)]])


def finish(lam, m1, m2, t, eps, W, ell, G, scale, tau, lr, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """bsc_glm_fullrank_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = elbo_and_grad(lam, eps, W, ell, G, scale, tau)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr, beta1, beta2, adam_eps)
    return lam2, m1, m2, elbo, grad


def step(link, lam, m1, m2, t, X, y, S, seed, n_total, lr, tau=1.0):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as
    GLMReparamSVI(covariance="full") does it.  Returns (lam, m1, m2, elbo, grad)."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W = draw(lam, eps)
    ell, G = mf.glm_data_pass(link, X, y, W)
    return finish(lam, m1, m2, t, eps, W, ell, G, n_total / B, tau, lr)


def elbo_fixed_draws(link, lam, eps, X, y, scale, tau):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of
    the draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    D = eps.shape[1]
    mu, L = unpack(lam, D)
    W = mu[None, :] + eps @ L.T
    Lg = np.asarray(X, np.float64) @ W.T
    A, _ = mf.log_partition(link, Lg)
    ell = (np.asarray(y, np.float64)[:, None] * Lg - A).sum(axis=0)
    f = scale * ell - 0.5 * tau * (W * W).sum(axis=1)
    return f.mean() + 0.5 * D * math.log(tau / (2.0 * math.pi)) + lam[diag_slots(D)].sum() + 0.5 * D * (1.0 + LOG_2PI)


# ---- the convergence experiment: AR(0.9) features, Laplace covariance at the MAP as the yardstick ---------------

def ar_glm_design(link, B, D, seed):
    """AR(0.9) features with unit marginal variance (neighbouring columns correlated 0.9, the posterior of w with
    them), w* = N(0, 1) / 2, y ~ Bernoulli(sigmoid(x . w*)) or y ~ Poisson(exp(0.5 x . w*))."""
    r = np.random.RandomState(seed)
    X = np.empty((B, D))
    X[:, 0] = r.standard_normal(B)
    for d in range(1, D):
        X[:, d] = 0.9 * X[:, d - 1] + math.sqrt(1.0 - 0.81) * r.standard_normal(B)
    l = X @ (r.standard_normal(D) / 2.0)
    if link == "logistic":
        y = r.uniform(size=B) < 1.0 / (1.0 + np.exp(-l))
    else:
        y = r.poisson(np.exp(0.5 * l))
    return X.astype(np.float32), y.astype(np.float32)


def laplace(link, X, y, tau=1.0, scale=1.0):
    """(w_MAP, H^{-1}) of log p(y, w) = scale sum_n [y_n l_n - A(l_n)] - tau/2 |w|^2 by Newton's method (concave:
    H = scale X^T diag A''(l) X + tau I is positive definite), float64."""
    X64, y64 = np.asarray(X, np.float64), np.asarray(y, np.float64)
    D = X64.shape[1]
    w = np.zeros(D)
    for _ in range(100):
        l = X64 @ w
        _, dA = mf.log_partition(link, l)
        d2A = dA * (1.0 - dA) if link == "logistic" else dA
        grad = scale * (X64.T @ (y64 - dA)) - tau * w
        H = scale * (X64.T * d2A[None, :]) @ X64 + tau * np.eye(D)
        delta = np.linalg.solve(H, grad)
        w = w + delta
        if np.abs(delta).max() < 1e-13:
            break
    l = X64 @ w
    _, dA = mf.log_partition(link, l)
    d2A = dA * (1.0 - dA) if link == "logistic" else dA
    H = scale * (X64.T * d2A[None, :]) @ X64 + tau * np.eye(D)
    return w, np.linalg.inv(H)


def covariance_error(C, exact):
    """Relative Frobenius error."""
    return float(np.linalg.norm(C - exact) / np.linalg.norm(exact))
