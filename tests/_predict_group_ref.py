"""Float64 numpy restatement of the grouped posterior predictive (include/bayesic_hip.h: bsc_predict_pass_groups;
bayesic_amd/svi/predict.py for HierGLMReparamSVI):

    l[n,s] = x_n . w_s + Bt[row(g_n), s] + o_n,      row(-1) = J (a group not seen in training), row(j) = j

and everything after l as tests/_predict_ref.py, whose log densities, log-mean-exp, Poisson moments and error factor are
used by import (the logistic variance is restated in a form that survives l = 80: ``moments``); the logits with the intercept are tests/_glm_group_ref.logits on the table's first S columns, its row J
standing in for the id -1.  Noise comes from the oracle by import (Philox stream 2, step 0)."""
import numpy as np
from scipy.special import expit

import _glm_group_ref as grp
import _glm_ref as glm
import _predict_ref as pref
from oracle import philox

EPS = pref.EPS
CODE = pref.CODE
FAMILIES = ("logistic", "poisson")


def table_ld(S):
    return 16 * ((S + 15) // 16)


def table(b, b_new):
    """Bt float32 [J + 1, ldb] from b [S, J] and b_new [S]: Bt[j, s] = b[s, j], row J = b_new, padding zero."""
    S, J = b.shape
    Bt = np.zeros((J + 1, table_ld(S)), np.float32)
    Bt[:J, :S] = np.asarray(b, np.float32).T
    Bt[J, :S] = np.asarray(b_new, np.float32)
    return Bt


def rows_of(g, J):
    """Table rows of the ids: -1 -> J."""
    g = np.asarray(g)
    return np.where(g == -1, J, g)


def logits(X, g, W, Bt, offset=None):
    """[B, S]: float32 operands, float64 arithmetic."""
    S = np.asarray(W).shape[0]
    J = Bt.shape[0] - 1
    return grp.logits(X, rows_of(g, J), W, np.asarray(Bt)[:, :S].T, offset)


def moments(family, L):
    """mu(l) and v(l) per (row, draw).  The logistic variance is sigmoid(l) sigmoid(-l): _predict_ref.moments' mu (1 - mu)
    cancels to exactly 0 in float64 from l = 37 on, and the intercept alone reaches l = 80 here."""
    if family == "logistic":
        mu = expit(L)
        return mu, mu * expit(-L)
    return pref.moments(family, L)


def dmu(family, L):
    """mu'(l): v for both families."""
    return moments(family, L)[1]


def predict_from_logits(family, L, y=None):
    mu, v = moments(family, L)
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = pref.log_mean_exp(pref.log_p(family, L, y))
        out["lpd_sum"] = out["lpd"].sum()
    return out


def predict(family, X, g, W, Bt, y=None, offset=None):
    """dict(mean, var[, lpd, lpd_sum]) in float64, as _predict_ref.predict."""
    return predict_from_logits(family, logits(X, g, W, Bt, offset), y)


def magnitude(X, g, W, Bt, offset=None):
    """a = |X| |W|^T + |b_s[g_n]| + |o_n|: what the float32 rounding of l scales with."""
    a = grp.logits(np.abs(np.asarray(X, np.float32)), rows_of(g, Bt.shape[0] - 1), np.abs(np.asarray(W, np.float32)),
                   np.abs(np.asarray(Bt))[:, :np.asarray(W).shape[0]].T, None if offset is None else np.abs(offset))
    return a


def bounds(family, X, g, W, Bt, y=None, offset=None):
    """_predict_ref.bounds with the magnitude term above (the same formulas and the same factor EPS)."""
    L = logits(X, g, W, Bt, offset)
    a = magnitude(X, g, W, Bt, offset)
    mu, v = moments(family, L)
    d1 = np.abs(dmu(family, L))
    e_mu = EPS * (d1 * a + np.abs(mu))
    mean = mu.mean(axis=1)
    e_v = EPS * (np.abs(1.0 - 2.0 * mu) * d1 * a + v) if family == "logistic" else e_mu
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = np.asarray(y, np.float64)[:, None]
        A, _ = glm.log_partition(family, L)
        out["lpd"] = (EPS * (np.abs(y64 * L) + A + 1.0)).max(axis=1)
        out["lpd_sum"] = out["lpd"].sum()
    return out


def predict_f32(family, X, g, W, Bt, y=None, offset=None):
    """The same formulas evaluated naively in float32, term after term (what a device pass may do at worst)."""
    X, W, Bt = (np.asarray(a, np.float32) for a in (X, W, Bt))
    B, D = X.shape
    S, J = W.shape[0], Bt.shape[0] - 1
    L = np.zeros((B, S), np.float32)
    for d in range(D):
        L += X[:, d:d + 1] * W[None, :, d]
    if offset is not None:
        L += np.asarray(offset, np.float32)[:, None]
    L += Bt[rows_of(g, J), :S]
    one = np.float32(1.0)
    if family == "logistic":
        e = np.exp(-np.abs(L)).astype(np.float32)
        mu = (np.where(L >= 0, one, e) / (one + e)).astype(np.float32)
        v = (e / ((one + e) * (one + e))).astype(np.float32)
        A = (np.maximum(L, np.float32(0)) + np.log1p(e)).astype(np.float32)
    else:
        mu = v = A = np.exp(L).astype(np.float32)
    mean = (mu.sum(axis=1, dtype=np.float32) / np.float32(S)).astype(np.float32)
    m2 = ((mu - mean[:, None]) ** 2).sum(axis=1, dtype=np.float32)
    out = dict(mean=mean, var=((v.sum(axis=1, dtype=np.float32) + m2) / np.float32(S)).astype(np.float32))
    if y is not None:
        from scipy.special import gammaln
        y32 = np.asarray(y, np.float32)
        lp = (y32[:, None] * L - A).astype(np.float32)
        mx = lp.max(axis=1)
        lpd = (mx + np.log(np.exp(lp - mx[:, None]).sum(axis=1, dtype=np.float32)) - np.float32(np.log(S))).astype(np.float32)
        if family == "poisson":
            lpd = (lpd - gammaln(y32.astype(np.float64) + 1.0).astype(np.float32)).astype(np.float32)
        out["lpd"] = lpd
        out["lpd_sum"] = lpd.astype(np.float64).sum()
    return out


def posterior_draws(lam, D, J, S, seed):
    """svi/predict.py's draws for the hierarchy: eps [S, D + J + 2] on Philox stream 2, step 0; columns 0 .. D + J go
    through z = m + e^rho eps over z = [w | b | zeta]; the last column is the unseen group's normal,
    b_new,s = e^{-zeta_s / 2} eps_s.  Returns (W float32 [S, D], Bt float32 [J + 1, ldb])."""
    lam = np.asarray(lam, np.float64)
    P = D + J + 1
    eps = philox.normal_draws(seed, S, P + 1, stream=pref.STREAM, step=0)
    z = lam[None, :P] + np.exp(lam[None, P:]) * eps[:, :P]
    b_new = np.exp(-0.5 * z[:, P - 1]) * eps[:, P]
    return z[:, :D].astype(np.float32), table(z[:, D:D + J], b_new)
