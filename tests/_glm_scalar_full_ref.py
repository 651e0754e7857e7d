"""Float64 numpy restatement of one update of the full-covariance Gaussian guide of the three regression families with a
learned scalar behind the weights (include/bayesic_hip.h, bsc_glm_scalar_fullrank_update; svi/glm_nb.py,
svi/glm_gamma.py, svi/glm_weibull.py with covariance="full"): q(z) = N(mu, L L^T) over z = [w (D) | tau], P = D + 1,
L lower-triangular with L_ii = e^{rho_i}, lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal
(P(P+1)/2)], rho_i in the diagonal slots.  The layout helpers are tests/_glm_full_ref.py's at width P, the noise, the
prior of tau and Adam tests/_glm_nb_ref.py's, the data passes the three families' own (tests/_glm_nb_ref.py,
tests/_glm_gamma_ref.py, tests/_glm_weibull_ref.py), all by import."""
import math

import numpy as np
from scipy.special import digamma, gammaln

from oracle import svi

import _glm_full_ref as fr
import _glm_gamma_ref as gamma
import _glm_nb_ref as nb
import _glm_ref as glm
import _glm_weibull_ref as weibull

LOG_2PI = fr.LOG_2PI
FAMILIES = ("negbin", "gamma", "weibull")
FAMILY_REF = {"negbin": nb, "gamma": gamma, "weibull": weibull}

n_lam = fr.n_lam                    # at width P
diag_slots = fr.diag_slots
unpack = fr.unpack
pack = fr.pack
init_lam = fr.init_lam              # the drivers' default at width P: mu = 0 (tau = 0), rho = log 0.1
from_mean_field = fr.from_mean_field
to_mean_field = fr.to_mean_field
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1], stream 0 in the columns of w, stream 1 in tau's
covariance_error = fr.covariance_error


def draw(lam, eps):
    """(W [S, D] float32, logscalar [S] float32) from eps [S, P]: z_s = mu + L eps_s rounded to float32 (what the pass
    reads and the finish uses)."""
    z = fr.draw(lam, eps)
    return z[:, :-1], z[:, -1]


# ---- the finish -----------------------------------------------------------------------------------------------------

def elbo_and_grad(lam, eps, W, logscalar, ell, G, T, scale, prec=1.0, a0=1.0, b0=1.0):
    """_glm_nb_ref.elbo_and_grad extended to L: g_s = [scale G_s - prec w_s | scale T_s + a0 - b0 e^{tau_s}] (W and tau
    as given: the device's are float32-rounded), d/d mu = mean_s g_s, d/d L_ij = mean_s g_si eps_sj (j < i),
    d/d rho_i = mean_s g_si eps_si e^{rho_i} + 1; the ELBO is the mean-field restatement's quantity."""
    lam = np.asarray(lam, np.float64)
    S, P = eps.shape
    D = P - 1
    rho = lam[diag_slots(P)]
    w, tau = np.asarray(W, np.float64), np.asarray(logscalar, np.float64)
    f = scale * np.asarray(ell, np.float64) - 0.5 * prec * (w * w).sum(axis=1) + nb.log_prior_tau(tau, a0, b0)
    elbo = f.mean() + 0.5 * D * math.log(prec / (2.0 * math.pi)) + rho.sum() + 0.5 * P * (1.0 + LOG_2PI)
    g = np.concatenate([scale * np.asarray(G, np.float64) - prec * w,
                        (scale * np.asarray(T, np.float64) + a0 - b0 * np.exp(tau))[:, None]], axis=1)
    gL = (g.T @ eps) / S
    d = np.arange(P)
    gL[d, d] = (g * eps).mean(axis=0) * np.exp(rho) + 1.0
    return elbo, np.concatenate([g.mean(axis=0), gL[np.tril_indices(P)]])


def finish(lam, m1, m2, t, eps, W, logscalar, ell, G, T, scale, prec, a0, b0, lr):
    """bsc_glm_scalar_fullrank_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = elbo_and_grad(lam, eps, W, logscalar, ell, G, T, scale, prec, a0, b0)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr)
    return lam2, m1, m2, elbo, grad


def step(family, lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None,
         lean=False):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> the family's pass -> finish), as the three
    drivers do it with covariance="full"; y is the family's response (Weibull: signed).  ``lean``: the pass is
    ``loglik`` below on the same float32 draws -- the same numbers without the bound quantities the families' data_pass
    forms beside them (tests/test_glm_scalar_full_cpu.py holds the two together), for the runs of thousands of steps."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logscalar = draw(lam, eps)
    if lean:
        ell, G, T = loglik(family, X, y, W, logscalar, offset, weights)
    else:
        ell, G, T = FAMILY_REF[family].data_pass(X, y, W, logscalar, offset, weights)
    return finish(lam, m1, m2, t, eps, W, logscalar, ell, G, T, n_total / B, prec, a0, b0, lr)


def mean_field_step(family, lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None,
                    weights=None, lean=False):
    """The family's own mean-field stepper (lam = [m | rho]); ``lean`` as in ``step``."""
    if not lean:
        return FAMILY_REF[family].step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec, a0, b0, offset, weights)
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logscalar = nb.draw(lam, eps)
    ell, G, T = loglik(family, X, y, W, logscalar, offset, weights)
    return nb.finish(lam, m1, m2, t, eps, W, logscalar, ell, G, T, n_total / B, prec, a0, b0, lr)


# ---- the smooth functions: everything float64, nothing rounded ---------------------------------------------------

def loglik(family, X, y, w, tau, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]) of the family's data pass with every operand taken as it is given (float64 draws are
    NOT rounded to float32, unlike the families' data_pass): a smooth function of (w, tau).  At float32-valued operands
    it is data_pass (tests/test_glm_scalar_full_cpu.py).  The negative binomial's ell leaves -sum v lnGamma(y + 1)
    out, as its pass does."""
    X64, y64 = np.asarray(X, np.float64), np.asarray(y, np.float64)[:, None]
    w, tau = np.asarray(w, np.float64), np.asarray(tau, np.float64)[None, :]
    l = X64 @ w.T
    if offset is not None:
        l = l + np.asarray(offset, np.float64)[:, None]
    v = np.ones(X64.shape[0]) if weights is None else np.asarray(weights, np.float64)
    keep = v > 0.0
    l, y64, v = l[keep], y64[keep], v[keep][:, None]
    e = np.exp(tau)
    if family == "negbin":
        u = l - tau
        sp, sg = glm.log_partition("logistic", u)
        r = v * (y64 - (y64 + e) * sg)
        t_ell = v * (gammaln(y64 + e) - gammaln(e) + y64 * u - (y64 + e) * sp)
        t_T = v * (e * (digamma(y64 + e) - digamma(e)) - e * sp) - r
    elif family == "gamma":
        c_a, c_1 = gamma.shape_constants(e)
        ly = np.log(y64)
        q = y64 * np.exp(-l)
        r = v * e * (q - 1.0)
        t_ell = v * (c_a + e * (ly - l - q) - ly)
        t_T = v * e * (c_1 + ly - l - q)
    elif family == "weibull":
        dl = (y64 > 0).astype(np.float64)
        ly = np.log(np.abs(y64))
        z = e * (ly - l)
        ez = np.exp(z)
        r = v * e * (ez - dl)
        t_ell = v * (dl * (tau + z - ly) - ez)
        t_T = v * (dl * (1.0 + z) - z * ez)
    else:
        raise ValueError(family)
    return t_ell.sum(axis=0), r.T @ X64[keep], t_T.sum(axis=0)


def elbo_fixed_draws(family, lam, eps, X, y, scale, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of the
    draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    P = eps.shape[1]
    D = P - 1
    mu, L = unpack(lam, P)
    z = mu[None, :] + eps @ L.T
    w, tau = z[:, :D], z[:, D]
    ell = loglik(family, X, y, w, tau, offset, weights)[0]
    f = scale * ell - 0.5 * prec * (w * w).sum(axis=1) + nb.log_prior_tau(tau, a0, b0)
    return f.mean() + 0.5 * D * math.log(prec / (2.0 * math.pi)) + lam[diag_slots(P)].sum() + 0.5 * P * (1.0 + LOG_2PI)


# ---- the convergence experiment: an intercept and AR(0.9) features, Laplace covariance at the MAP as the yardstick -

def log_joint_grad(family, z, X, y, prec=1.0, a0=1.0, b0=1.0, scale=1.0, offset=None, weights=None):
    """(log p(y, z) up to a constant, its gradient [P]) at z = [w | tau]."""
    D = X.shape[1]
    w, tau = z[:D], z[D]
    ell, G, T = loglik(family, X, y, w[None, :], np.array([tau]), offset, weights)
    f = scale * ell[0] - 0.5 * prec * (w @ w) + a0 * tau - b0 * np.exp(tau)
    return f, np.concatenate([scale * G[0] - prec * w, [scale * T[0] + a0 - b0 * np.exp(tau)]])


def log_joint_hessian(family, z, X, y, h=1e-5, **kw):
    """Central differences of the analytic gradient, symmetrised."""
    P = z.size
    H = np.empty((P, P))
    for i in range(P):
        e = np.zeros(P)
        e[i] = h
        H[i] = (log_joint_grad(family, z + e, X, y, **kw)[1] - log_joint_grad(family, z - e, X, y, **kw)[1]) / (2 * h)
    return 0.5 * (H + H.T)


@np.errstate(over="ignore", invalid="ignore")
def laplace(family, X, y, prec=1.0, a0=1.0, b0=1.0, scale=1.0, offset=None, weights=None):
    """(z_MAP, (-H)^{-1}) of the log-joint in z = [w | tau], float64: damped Newton from z = 0 (the step is halved until
    the log-joint rises), with the Hessian by central differences of the analytic gradient."""
    kw = dict(prec=prec, a0=a0, b0=b0, scale=scale, offset=offset, weights=weights)
    z = np.zeros(X.shape[1] + 1)
    f, g = log_joint_grad(family, z, X, y, **kw)
    for _ in range(200):                            # (an overshooting trial step may overflow: it is halved)
        H = log_joint_hessian(family, z, X, y, **kw)
        lo = np.linalg.eigvalsh(-H).min()
        if lo <= 0.0:                               # far from the mode: shift to positive definite
            H = H - (1e-3 - lo) * np.eye(z.size)
        delta = np.linalg.solve(-H, g)
        step_len = 1.0
        while True:
            f2, g2 = log_joint_grad(family, z + step_len * delta, X, y, **kw)
            if np.isfinite(f2) and f2 >= f:
                break
            step_len *= 0.5
            if step_len < 1e-10:
                break
        z, f, g = z + step_len * delta, f2, g2
        if np.abs(step_len * delta).max() < 1e-12:
            break
    assert np.abs(g).max() < 1e-6 * max(1.0, abs(f)), "laplace: the Newton iteration did not reach the mode"
    return z, np.linalg.inv(-log_joint_hessian(family, z, X, y, **kw))


def ar_weibull_design(B, D, seed, shape=1.5, censored=0.3):
    """An intercept column followed by D - 1 AR(0.9) features of unit marginal variance, w* = [0.5, N(0, 1) / 2],
    event times t ~ Weibull(shape, scale e^{x . w*}) and independent censoring times of the same law stretched by
    f = ((1 - c) / c)^{1 / shape}, so that a share c = ``censored`` of the rows is cut (P(f C < T) = 1 / (1 + f^shape)).
    Returns (X float32, y float32 signed: negative = right-censored)."""
    r = np.random.RandomState(seed)
    X = np.empty((B, D))
    X[:, 0] = 1.0
    X[:, 1] = r.standard_normal(B)
    for d in range(2, D):
        X[:, d] = 0.9 * X[:, d - 1] + math.sqrt(1.0 - 0.81) * r.standard_normal(B)
    w = np.concatenate([[0.5], r.standard_normal(D - 1) / 2.0])
    sc = np.exp(X @ w)
    t = sc * r.weibull(shape, B)
    c = sc * r.weibull(shape, B) * ((1.0 - censored) / censored) ** (1.0 / shape)
    y = np.where(c < t, -c, t)
    return X.astype(np.float32), y.astype(np.float32)
