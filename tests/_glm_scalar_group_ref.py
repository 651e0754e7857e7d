"""Float64 numpy restatement of the random-intercept routes of the families with a learned scalar
(include/bayesic_hip.h: bsc_glm_scalar_data_pass_groups, bsc_glm_scalar_hier_update, bsc_scalar_predict_pass_groups;
svi/hier_scalar.py):

    l[n,s] = x_n . w_s + b_s[g_n] + o_n,     y_n ~ F(l_ns, e^{tau_s}),     F in {negbin, gamma, weibull}
    stats  = [ell (S) | G (S D) | H (S J) | T (S)],   H[s,j] = sum_{n : g_n = j} r_ns,   T[s] = d ell[s] / d tau_s

under w ~ N(0, I / prec), b_j | zeta ~ N(0, e^{-zeta}), e^zeta ~ Gamma(ga0, gb0), e^tau ~ Gamma(a0, b0);
z = [w (D) | b (J) | zeta | tau], P = D + J + 2, lam = [m (P) | rho (P)].

NO NEW LINK MATH in the pass and its bounds: the intercept is a coefficient of the one-hot design, so the family's own
helper (tests/_glm_nb_ref.py, tests/_glm_gamma_ref.py, tests/_glm_weibull_ref.py) on [X | onehot(g, J)] and [W | Bm]
returns (ell, [G | H], T), and its bounds and predict_bounds on the same arguments give the error scales.  The finish
is the formulas of include/bayesic_hip.h restated; Adam and the noise come from the oracle.  ``loglik64`` restates the
three log densities in float64 WITHOUT rounding the draws to float32, for the one test that differentiates the ELBO
numerically; tests/test_glm_scalar_group_cpu.py ties it to the family helpers."""
import math

import numpy as np
from scipy.special import gammaln

import _glm_gamma_ref as gm
import _glm_group_ref as grp
import _glm_nb_ref as nb
import _glm_ref as glm
import _glm_weibull_ref as wb
from oracle import philox, svi

LOG_2PI = glm.LOG_2PI
FAMILIES = ("negbin", "gamma", "weibull")
CODE = {"negbin": 0, "gamma": 1, "weibull": 2}          # include/bayesic_hip.h: BSC_SCALAR_*
MOD = {"negbin": nb, "gamma": gm, "weibull": wb}
TAU_RANGE = {"negbin": (-2.5, 5.0), "gamma": (-2.5, 5.0), "weibull": (-2.0, 4.0)}     # the accuracy envelopes

onehot = grp.onehot
chunked = grp.chunked
unchunk = grp.unchunk


def design(X, g, J):
    """[X | onehot(g, J)] float32 [B, D + J]."""
    return np.concatenate([np.asarray(X, np.float32), onehot(g, J)], axis=1)


def draws(W, Bm):
    """[W | Bm] float32 [S, D + J]."""
    return np.concatenate([np.asarray(W, np.float32), np.asarray(Bm, np.float32)], axis=1)


# ---- the pass -------------------------------------------------------------------------------------------------------

def data_pass(fam, X, y, g, J, W, Bm, logtau, offset=None, weights=None):
    """(ell [S], G [S, D], H [S, J], T [S]): float32 operands, float64 arithmetic."""
    D = np.asarray(X).shape[1]
    ell, GH, T = MOD[fam].data_pass(design(X, g, J), y, draws(W, Bm), logtau, offset, weights)
    return ell, GH[:, :D], GH[:, D:], T


def bounds(fam, X, y, g, J, W, Bm, logtau, offset=None, weights=None):
    """(b_ell [S], b_T [S]): what the device's errors of ell and T are measured against, each times 2e-5."""
    b = MOD[fam].bounds(design(X, g, J), y, draws(W, Bm), logtau, offset, weights)
    return b[0], b[-1]


# ---- draws ----------------------------------------------------------------------------------------------------------

def init_lam(P):
    """The driver's default: m = 0, rho = log 0.1."""
    return grp.init_lam(P)


def noise(D, J, S, seed, step):
    """bsc_blr_noise(P - 1): [S, P], Philox stream 0 in the columns of w, b and zeta, stream 1 in tau's."""
    return np.concatenate([philox.normal_draws(seed, S, D + J + 1, stream=0, step=step),
                           philox.normal_draws(seed, S, 1, stream=1, step=step)], axis=1)


def draw(lam, eps, D, J):
    """(W [S, D] float32, Bm [S, J] float32, zeta [S] float64, logtau [S] float32): what the pass reads, and zeta as the
    finish forms it."""
    P = D + J + 2
    lam = np.asarray(lam, np.float64)
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    return z[:, :D].astype(np.float32), z[:, D:D + J].astype(np.float32), z[:, P - 2], z[:, P - 1].astype(np.float32)


# ---- the finish -----------------------------------------------------------------------------------------------------

def log_prior(w, b, zeta, tau, prec=1.0, a0=1.0, b0=1.0, ga0=1.0, gb0=1.0):
    """log p(z) per draw, every normaliser included."""
    D, J = w.shape[1], b.shape[1]
    ez = np.exp(zeta)
    c0 = (0.5 * D * math.log(prec / (2.0 * math.pi)) - 0.5 * J * LOG_2PI + ga0 * math.log(gb0) - math.lgamma(ga0)
          + a0 * math.log(b0) - math.lgamma(a0))
    return (c0 - 0.5 * prec * (w * w).sum(axis=1) + 0.5 * J * zeta - 0.5 * ez * (b * b).sum(axis=1) + ga0 * zeta
            - gb0 * ez + a0 * tau - b0 * np.exp(tau))


def elbo_and_grad(lam, eps, W, Bm, zeta, logtau, ell, G, H, T, scale, prec=1.0, a0=1.0, b0=1.0, ga0=1.0, gb0=1.0):
    lam = np.asarray(lam, np.float64)
    S, D = W.shape
    J = Bm.shape[1]
    P = D + J + 2
    rho = lam[P:]
    w, b, tau = np.asarray(W, np.float64), np.asarray(Bm, np.float64), np.asarray(logtau, np.float64)
    ez = np.exp(zeta)
    f = scale * ell + log_prior(w, b, zeta, tau, prec, a0, b0, ga0, gb0)
    elbo = f.mean() + rho.sum() + 0.5 * P * (1.0 + LOG_2PI)
    g = np.concatenate([scale * G - prec * w, scale * H - ez[:, None] * b,
                        (0.5 * J + ga0 - ez * (gb0 + 0.5 * (b * b).sum(axis=1)))[:, None],
                        (scale * T + a0 - b0 * np.exp(tau))[:, None]], axis=1)
    return elbo, np.concatenate([g.mean(axis=0), (g * eps).mean(axis=0) * np.exp(rho) + 1.0])


def finish(lam, m1, m2, t, eps, W, Bm, zeta, logtau, ell, G, H, T, scale, prec, a0, b0, ga0, gb0, lr):
    """bsc_glm_scalar_hier_update from given statistics.  Returns (lam', m1', m2', elbo, grad)."""
    elbo, grad = elbo_and_grad(lam, eps, W, Bm, zeta, logtau, ell, G, H, T, scale, prec, a0, b0, ga0, gb0)
    lam2, m1, m2 = svi.adam_ascent(np.asarray(lam, np.float64), grad, m1, m2, t, lr)
    return lam2, m1, m2, elbo, grad


def step(fam, lam, m1, m2, t, X, y, g, J, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, ga0=1.0, gb0=1.0,
         offset=None, weights=None, info=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as the drivers of
    svi/hier_scalar.py do it.  ``info`` (a dict) receives the draws and scale * mean_s b_ell[s], the size of the ELBO's
    data terms."""
    B, D = X.shape
    eps = noise(D, J, S, seed, t - 1)
    W, Bm, zeta, logtau = draw(lam, eps, D, J)
    ell, G, H, T = data_pass(fam, X, y, g, J, W, Bm, logtau, offset, weights)
    if info is not None:
        info.update(W=W, Bm=Bm, zeta=zeta, logtau=logtau,
                    size=n_total / B * bounds(fam, X, y, g, J, W, Bm, logtau, offset, weights)[0].mean())
    return finish(lam, m1, m2, t, eps, W, Bm, zeta, logtau, ell, G, H, T, n_total / B, prec, a0, b0, ga0, gb0, lr)


def loglik64(fam, L, y, tau):
    """sum_n log p(y_n | l_ns, e^{tau_s}) [S] in float64 from float64 l [B, S] and tau [S], in the forms of
    include/bayesic_hip.h (negbin: without -lnGamma(y + 1), as the pass leaves it out; weibull: y signed)."""
    y64 = np.asarray(y, np.float64)[:, None]
    tau = np.asarray(tau, np.float64)[None, :]
    e = np.exp(tau)
    if fam == "negbin":
        u = L - tau
        sp, _ = glm.log_partition("logistic", u)
        lp = gammaln(y64 + e) - gammaln(e) + y64 * u - (y64 + e) * sp
    elif fam == "gamma":
        ly = np.log(y64)
        lp = e * np.log(e) - gammaln(e) + e * (ly - L - y64 * np.exp(-L)) - ly
    else:
        ly = np.log(np.abs(y64))
        z = e * (ly - L)
        lp = (y64 > 0) * (tau + z - ly) - np.exp(z)
    return lp.sum(axis=0)


def elbo_fixed_draws(fam, lam, eps, X, y, g, J, scale, prec=1.0, a0=1.0, b0=1.0, ga0=1.0, gb0=1.0, offset=None):
    """The ELBO estimate as a smooth function of lam with the noise held fixed, all float64 (no float32 rounding of
    the draws): what the pathwise gradient is the derivative of."""
    lam = np.asarray(lam, np.float64)
    D = X.shape[1]
    P = D + J + 2
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    w, b, zeta, tau = z[:, :D], z[:, D:D + J], z[:, P - 2], z[:, P - 1]
    L = np.asarray(X, np.float64) @ w.T + b[:, np.asarray(g)].T
    if offset is not None:
        L = L + np.asarray(offset, np.float64)[:, None]
    f = scale * loglik64(fam, L, y, tau) + log_prior(w, b, zeta, tau, prec, a0, b0, ga0, gb0)
    return f.mean() + lam[P:].sum() + 0.5 * P * (1.0 + LOG_2PI)


# ---- a simulated grouped data set and its float64 fits (the end-to-end tests of both test files) ---------------------

FIT = dict(B=3000, B_test=1000, D=8, J=20, spread=0.8, steps=300, S=8, lr=0.05, seed=77, S_pred=32)


def simulate(fam, seed=5):
    """Train and test rows of one grouped data set with a KNOWN intercept spread FIT["spread"]: a dict of X, y (the
    signed response for weibull), g and their *_test twins.  negbin: phi = 3; gamma: alpha = 3; weibull: k = 1.5, three rows in
    ten censored at a uniform fraction of their duration."""
    rs = np.random.RandomState(seed)
    n, D, J = FIT["B"] + FIT["B_test"], FIT["D"], FIT["J"]
    X = (rs.standard_normal((n, D)) / math.sqrt(D)).astype(np.float32)
    g = rs.randint(J, size=n).astype(np.int32)
    l = X.astype(np.float64) @ (0.5 * rs.standard_normal(D)) + FIT["spread"] * rs.standard_normal(J)[g]
    if fam == "negbin":
        y = rs.negative_binomial(3, 3.0 / (3.0 + np.exp(l)))
    elif fam == "gamma":
        y = np.maximum(rs.gamma(3.0, np.exp(l) / 3.0), 1e-30)
    else:
        t = np.maximum(np.exp(l) * rs.weibull(1.5, n), 1e-30)
        cens = rs.uniform(size=n) < 0.3
        y = np.where(cens, -t * rs.uniform(0.1, 1.0, n), t)
    y = y.astype(np.float32)
    k = FIT["B"]
    return dict(X=X[:k], y=y[:k], g=g[:k], X_test=X[k:], y_test=y[k:], g_test=g[k:])


def fit(fam, data, grouped=True):
    """lam after FIT["steps"] float64 updates from the default start, the drivers' default priors (a0 = 1, b0 = 0.1,
    group_a0 = group_b0 = 1, prior_precision = 1); ``grouped=False``: the family's own stepper without the ids."""
    X, y, g = data["X"], data["y"], data["g"]
    B, D = X.shape
    J, S, seed, lr = FIT["J"], FIT["S"], FIT["seed"], FIT["lr"]
    lam = init_lam(D + J + 2) if grouped else MOD[fam].init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, FIT["steps"] + 1):
        if grouped:
            lam, m1, m2, _, _ = step(fam, lam, m1, m2, t, X, y, g, J, S, seed, float(B), lr, 1.0, 1.0, 0.1, 1.0, 1.0)
        else:
            lam, m1, m2, _, _ = MOD[fam].step(lam, m1, m2, t, X, y, S, seed, float(B), lr, 1.0, 1.0, 0.1)
    return lam


def heldout(fam, data, lam, grouped=True, known=True):
    """Mean held-out lpd per test row under FIT["S_pred"] predictive draws; ``known=False``: every id is -1."""
    X, y, g = data["X_test"], data["y_test"], data["g_test"]
    D, J, S, seed = X.shape[1], FIT["J"], FIT["S_pred"], FIT["seed"]
    if not grouped:
        W, logtau = MOD[fam].posterior_draws(lam, D, S, seed)
        return float(MOD[fam].predict(X, W, logtau, y)["lpd"].mean())
    W, Bm, b_new, logtau = posterior_draws(lam, D, J, S, seed)
    ids = g if known else np.full(len(g), -1, np.int32)
    return float(predict(fam, X, ids, J, W, Bm, b_new, logtau, y)["lpd"].mean())


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, J, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, P + 1].  Returns (W float32 [S, D], Bm float32 [S, J], b_new
    float32 [S], logtau float32 [S])."""
    P = D + J + 2
    eps = philox.normal_draws(seed, S, P + 1, stream=2, step=0)
    lam = np.asarray(lam, np.float64)
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps[:, :P]
    b_new = np.exp(-0.5 * z[:, P - 2]) * eps[:, P]
    return (z[:, :D].astype(np.float32), z[:, D:D + J].astype(np.float32), b_new.astype(np.float32),
            z[:, P - 1].astype(np.float32))


def table(Bm, b_new):
    """Bt float32 [J + 1, ldb]: Bt[j, s] = Bm[s, j], row J = b_new, ldb = 16 ceil(S / 16), padding zero."""
    S, J = Bm.shape
    Bt = np.zeros((J + 1, 16 * ((S + 15) // 16)), np.float32)
    Bt[:J, :S] = Bm.T
    Bt[J, :S] = b_new
    return Bt


def _with_new(g, J, Bm, b_new):
    """ids with -1 -> J and the draws with b_new as column J: the one-hot design at J + 1 groups."""
    g = np.asarray(g)
    return np.where(g < 0, J, g), np.concatenate([Bm, np.asarray(b_new, np.float32)[:, None]], axis=1)


def predict(fam, X, g, J, W, Bm, b_new, logtau, y=None, offset=None, weights=None):
    g1, B1 = _with_new(g, J, Bm, b_new)
    return MOD[fam].predict(design(X, g1, J + 1), draws(W, B1), logtau, y, offset, weights)


def predict_bounds(fam, X, g, J, W, Bm, b_new, logtau, y=None, offset=None, weights=None):
    g1, B1 = _with_new(g, J, Bm, b_new)
    return MOD[fam].predict_bounds(design(X, g1, J + 1), draws(W, B1), logtau, y, offset, weights)
