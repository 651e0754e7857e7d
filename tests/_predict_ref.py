"""Float64 numpy restatement of the posterior predictive (include/bayesic_hip.h: bsc_predict_pass;
bayesic_amd/svi/predict.py).  Noise comes from the oracle by import (Philox stream 2, step 0), the log-partition
functions from tests/_glm_ref.py, the full guide's layout from tests/_fullrank_ref.py."""
import math

import numpy as np
from scipy.special import gammaln

import _fullrank_ref as fr
import _glm_ref as glm
from oracle import philox

LOG_2PI = math.log(2.0 * math.pi)
STREAM = 2
FAMILIES = ("gaussian", "logistic", "poisson")
CODE = {"gaussian": 0, "logistic": 1, "poisson": 2}


def logits(X, W):
    """l = X W^T: float32 operands, float64 arithmetic."""
    return np.asarray(X, np.float32).astype(np.float64) @ np.asarray(W, np.float32).astype(np.float64).T


def moments(family, L, logvar=None):
    """mu(l) and v(l) per (row, draw)."""
    if family == "gaussian":
        return L.copy(), np.broadcast_to(np.exp(np.asarray(logvar, np.float64))[None, :], L.shape).copy()
    _, mu = glm.log_partition(family, L)
    return mu, (mu * (1.0 - mu) if family == "logistic" else mu.copy())


def dmu(family, L):
    """mu'(l): 1, mu (1 - mu), mu."""
    if family == "gaussian":
        return np.ones_like(L)
    _, mu = glm.log_partition(family, L)
    return mu * (1.0 - mu) if family == "logistic" else mu


def log_p(family, L, y, logvar=None):
    """log p(y | l) per (row, draw); the Poisson constant lnGamma(y + 1) included."""
    y = np.asarray(y, np.float64)[:, None]
    if family == "gaussian":
        lv = np.asarray(logvar, np.float64)[None, :]
        return -0.5 * (lv + LOG_2PI) - 0.5 * np.exp(-lv) * (y - L) ** 2
    A, _ = glm.log_partition(family, L)
    out = y * L - A
    return out - gammaln(y + 1.0) if family == "poisson" else out


def log_mean_exp(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(family, X, W, logvar=None, y=None):
    """dict(mean, var[, lpd, lpd_sum]) in float64; var by the law of total variance, centred."""
    L = logits(X, W)
    mu, v = moments(family, L, logvar)
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = log_mean_exp(log_p(family, L, y, logvar))
        out["lpd_sum"] = out["lpd"].sum()
    return out


def posterior_draws(kind, lam, D, S, seed):
    """svi/predict.py's draws: kind = "glm" | "diag" | "full".  Returns (W float32 [S, D], logvar float32 [S] | None)."""
    lam = np.asarray(lam, np.float64)
    if kind == "glm":
        eps = philox.normal_draws(seed, S, D, stream=STREAM, step=0)
        return (lam[None, :D] + np.exp(lam[D:2 * D])[None, :] * eps).astype(np.float32), None
    eps = philox.normal_draws(seed, S, D + 1, stream=STREAM, step=0)
    if kind == "diag":
        W = lam[None, :D] + np.exp(lam[D:2 * D])[None, :] * eps[:, :D]
        return W.astype(np.float32), (lam[2 * D] + np.exp(lam[2 * D + 1]) * eps[:, D]).astype(np.float32)
    mu, L = fr.unpack(lam, D + 1)
    z = mu[None, :] + eps @ L.T
    return z[:, :D].astype(np.float32), z[:, D].astype(np.float32)


# ---- error bounds of the device pass, from float64 reference quantities and the project's factor 2e-5 ------------
EPS = 2e-5


def bounds(family, X, W, logvar=None, y=None):
    """Per-row bounds on |device - reference| for mean, var and lpd (tests/test_predict_gpu.py's docstring)."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    W64 = np.asarray(W, np.float32).astype(np.float64)
    L = X64 @ W64.T
    a = np.abs(X64) @ np.abs(W64).T
    mu, v = moments(family, L, logvar)
    d1 = np.abs(dmu(family, L))
    S = L.shape[1]
    e_mu = EPS * (d1 * a + np.abs(mu))                       # per-draw error of mu
    mean = mu.mean(axis=1)
    if family == "gaussian":
        e_v = EPS * v
    elif family == "logistic":
        e_v = EPS * (np.abs(1.0 - 2.0 * mu) * d1 * a + v)    # v = mu (1 - mu): dv/dl = (1 - 2 mu) mu'
    else:
        e_v = e_mu
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = np.asarray(y, np.float64)[:, None]
        if family == "gaussian":
            lv = np.asarray(logvar, np.float64)[None, :]
            r = y64 - L
            e = EPS * (np.exp(-lv) * (np.abs(r) * (a + np.abs(y64)) + r * r) + np.abs(lv) + 1.0)
        else:
            A, _ = glm.log_partition(family, L)
            e = EPS * (np.abs(y64 * L) + A + 1.0)
        out["lpd"] = e.max(axis=1)
        out["lpd_sum"] = out["lpd"].sum()
    return out
