"""Float64 numpy restatement of the GLM pass with per-row offsets and weights (include/bayesic_hip.h:
bsc_glm_data_pass_obs, bsc_predict_pass_offset; svi/glm.py):

    l[n,s] = x_n . w_s + o[n],   ell[s] = sum_n v[n] (y[n] l[n,s] - A(l[n,s])),   G[s,:] = sum_n v[n] (y[n] - A'(l[n,s])) x_n

with rows of weight 0 dropped by a select (their link value may be infinite).  The link functions, the draws, the
finish and Adam are tests/_glm_ref.py's, by import."""
import numpy as np

import _glm_ref as glm
import _predict_ref as pred


def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def logits(X, W, offset=None):
    L = _f64(X) @ _f64(W).T
    return L if offset is None else L + _f64(offset)[:, None]


def data_pass(link, X, y, W, offset=None, weights=None):
    """(ell [S], G [S, D]): float32 operands, float64 arithmetic."""
    X64, y64 = _f64(X), _f64(y)[:, None]
    L = logits(X, W, offset)
    v = np.ones(X64.shape[0]) if weights is None else _f64(weights)
    on = v > 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        A, dA = glm.log_partition(link, L)
        t_ell = np.where(on[:, None], v[:, None] * (y64 * L - A), 0.0)
        t_res = np.where(on[:, None], v[:, None] * (y64 - dA), 0.0)
    return t_ell.sum(axis=0), t_res.T @ X64


def ell_bound(link, X, y, W, offset=None, weights=None):
    """The quantity the device's ell error is measured against: sum_n v_n (|y_n l_ns| + A(l_ns) + 1), rows of weight 0
    left out."""
    L = logits(X, W, offset)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = v > 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        A, _ = glm.log_partition(link, L)
        t = np.where(on[:, None], v[:, None] * (np.abs(_f64(y)[:, None] * L) + A + 1.0), 0.0)
    return t.sum(axis=0)


def data_pass_f32(link, X, y, W, offset=None, weights=None):
    """The same formulas evaluated naively in float32, row after row (what a device pass may do at worst)."""
    X, y, W = np.asarray(X, np.float32), np.asarray(y, np.float32), np.asarray(W, np.float32)
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, np.float32) if offset is None else np.asarray(offset, np.float32)
    v = np.ones(B, np.float32) if weights is None else np.asarray(weights, np.float32)
    ell, G = np.zeros(S, np.float32), np.zeros((S, D), np.float32)
    one = np.float32(1.0)
    for n in range(B):
        if not v[n] > 0:
            continue
        l = (X[n][None, :] * W).sum(axis=1, dtype=np.float32) + o[n]
        if link == "logistic":
            e = np.exp(-np.abs(l)).astype(np.float32)
            a = (np.maximum(l, np.float32(0)) + np.log1p(e)).astype(np.float32)
            da = (np.where(l >= 0, one, e) / (one + e)).astype(np.float32)
        else:
            a = da = np.exp(l).astype(np.float32)
        ell += v[n] * (y[n] * l - a)
        G += (v[n] * (y[n] - da))[:, None] * X[n][None, :]
    return ell, G


def expand_binomial(X, k, n):
    """Rows (x, k successes of n trials) as n Bernoulli rows each: (X', y')."""
    k, n = np.asarray(k, int), np.asarray(n, int)
    rows = np.repeat(np.arange(X.shape[0]), n)
    y = np.concatenate([np.r_[np.ones(ki), np.zeros(ni - ki)] for ki, ni in zip(k, n)]) if len(k) else np.zeros(0)
    return np.asarray(X)[rows], y.astype(np.float32)


def step(link, lam, m1, m2, t, X, y, S, seed, n_total, lr, tau=1.0, offset=None, weights=None):
    """_glm_ref.glm_step with the offset and the weights in the pass; the scale stays n_total / B."""
    B, D = X.shape
    eps = glm.noise(D, S, seed, t - 1)
    W = glm.draw(lam, eps)
    ell, G = data_pass(link, X, y, W, offset, weights)
    return glm.finish(lam, m1, m2, t, eps, W, ell, G, n_total / B, tau, lr)


# ---- predictive ---------------------------------------------------------------------------------------------------

def predict(family, X, W, y=None, offset=None, weights=None):
    """_predict_ref.predict with l + o; lpd stays per row, lpd_sum = sum_n v_n lpd_n with weights."""
    L = logits(X, W, offset)
    mu, v = pred.moments(family, L)
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = pred.log_mean_exp(pred.log_p(family, L, y))
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(family, X, W, y=None, offset=None, weights=None):
    """_predict_ref.bounds restated for l = x . w + o: the offset is one more float32 term of the logit, so a_ns gains
    |o_n|; with weights the bound of lpd_sum is sum_n v_n bound(lpd_n) plus 2e-5 of sum_n v_n |lpd_n| for the product
    (float64 on the device: generous)."""
    X64, W64 = _f64(X), _f64(W)
    L = logits(X, W, offset)
    a = np.abs(X64) @ np.abs(W64).T
    if offset is not None:
        a = a + np.abs(_f64(offset))[:, None]
    mu, v = pred.moments(family, L)
    d1 = np.abs(pred.dmu(family, L))
    EPS = pred.EPS
    e_mu = EPS * (d1 * a + np.abs(mu))
    mean = mu.mean(axis=1)
    e_v = EPS * (np.abs(1.0 - 2.0 * mu) * d1 * a + v) if family == "logistic" else e_mu
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        A, _ = glm.log_partition(family, L)
        e = EPS * (np.abs(_f64(y)[:, None] * L) + A + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
