"""Float64 numpy restatement of one update of the full-covariance Gaussian guide (include/bayesic_hip.h,
bsc_blr_fullrank_update): q(z) = N(mu, L L^T) over z = [w (D) | xi], L lower-triangular with L_ii = e^{rho_i},
lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal (P(P+1)/2)], rho_i in the diagonal slots."""
import math

import numpy as np

from oracle import philox, svi

LOG_2PI = math.log(2.0 * math.pi)


def n_lam(D):
    P = D + 1
    return P + P * (P + 1) // 2


def diag_slots(P):
    i = np.arange(P)
    return P + i * (i + 1) // 2 + i


def unpack(lam, P):
    """(mu [P], L [P, P]) with the diagonal exponentiated."""
    lam = np.asarray(lam, np.float64)
    L = np.zeros((P, P))
    L[np.tril_indices(P)] = lam[P:]
    d = np.arange(P)
    L[d, d] = np.exp(L[d, d])
    return lam[:P].copy(), L


def pack(mu, L):
    """Inverse of unpack (L's diagonal must be positive)."""
    P = len(mu)
    Lr = np.array(L, np.float64)
    d = np.arange(P)
    Lr[d, d] = np.log(Lr[d, d])
    return np.concatenate([np.asarray(mu, np.float64), Lr[np.tril_indices(P)]])


def init_lam(D):
    """The driver's default: mu = 0, rho = log 0.1, zero off-diagonal entries."""
    lam = np.zeros(n_lam(D))
    lam[diag_slots(D + 1)] = math.log(0.1)
    return lam


def from_mean_field(lam_mf, D):
    """[m | rho | a | b] -> the full layout with zero off-diagonal entries."""
    P = D + 1
    lam = np.zeros(n_lam(D))
    lam[:D], lam[D] = lam_mf[:D], lam_mf[2 * D]
    lam[diag_slots(P)] = np.concatenate([lam_mf[D:2 * D], [lam_mf[2 * D + 1]]])
    return lam


def nig_family(B, scale, D, alpha0=1.0, beta0=1.0):
    """Config 2 as a member of f(w, xi; Q) = c0 + c_xi xi + e^{-xi} (-s_q Q / 2 - k_w |w|^2 / 2 - beta)."""
    half = 0.5 * (scale * B + D)
    return (-half * LOG_2PI + alpha0 * math.log(beta0) - math.lgamma(alpha0), -half - alpha0, scale, 1.0, beta0)


def noise(D, S, seed, step):
    """bsc_blr_noise's [S, D+1]: stream 0 for w, stream 1 for xi."""
    return np.concatenate([philox.normal_draws(seed, S, D, stream=0, step=step),
                           philox.normal_draws(seed, S, 1, stream=1, step=step)], axis=1)


def draw(lam, eps):
    """z_s = mu + L eps_s -> (W float32 [S, D], xi [S])."""
    S, P = eps.shape
    mu, L = unpack(lam, P)
    z = mu[None, :] + eps @ L.T
    return z[:, :P - 1].astype(np.float32), z[:, P - 1].copy()


def family_f_and_g(W, xi, Q, G, family):
    """f_s and g_s = d f / d z at z_s = [w_s | xi_s] for the family (W as given: the device's are float32-rounded)."""
    c0, c_xi, s_q, k_w, beta = family
    S, D = W.shape
    W64 = np.asarray(W, np.float64)
    e = np.exp(-xi)
    inner = 0.5 * s_q * Q + 0.5 * k_w * (W64 * W64).sum(axis=1) + beta
    f = c0 + c_xi * xi - e * inner
    g = np.empty((S, D + 1))
    g[:, :D] = e[:, None] * (s_q * G - k_w * W64)
    g[:, D] = c_xi + e * inner
    return f, g


def estimate(lam, eps, f, g):
    """ELBO estimate and pathwise gradient (lam's layout) from f_s, g_s at z_s = mu + L eps_s."""
    S, P = eps.shape
    rho = np.asarray(lam, np.float64)[diag_slots(P)]
    elbo = f.mean() + rho.sum() + 0.5 * P * (1.0 + LOG_2PI)
    gL = (g.T @ eps) / S
    d = np.arange(P)
    gL[d, d] = (g * eps).mean(axis=0) * np.exp(rho) + 1.0
    return elbo, np.concatenate([g.mean(axis=0), gL[np.tril_indices(P)]])


def finish(lam, m1, m2, t, eps, W, xi, Q, G, family, lr, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """Gradient, ELBO and Adam step of bsc_blr_fullrank_update.  Returns (lam', m1', m2', elbo, grad)."""
    f, g = family_f_and_g(W, xi, Q, G, family)
    elbo, grad = estimate(lam, eps, f, g)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr, beta1, beta2, adam_eps)
    return lam2, m1, m2, elbo, grad


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, family=None, alpha0=1.0, beta0=1.0):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as BLRReparamSVI(covariance="full")
    does it.  Returns (lam, m1, m2, elbo, grad)."""
    B, D = X.shape
    if family is None:
        family = nig_family(B, n_total / B, D, alpha0, beta0)
    eps = noise(D, S, seed, t - 1)
    W, xi = draw(lam, eps)
    Q, G = svi.blr_data_pass(X, y, W)
    return finish(lam, m1, m2, t, eps, W, xi, Q, G, family, lr)
