"""Float64 numpy restatement of the softmax-regression pass and predictive (include/bayesic_hip.h:
bsc_softmax_data_pass, bsc_softmax_predict_pass; bayesic_amd/svi/softmax.py): labels y_n in {0 .. K-1}, weights
W[S, K, D] (flattened parameter p = k D + d), float32 operands, float64 arithmetic.  A row whose label is outside
[0, K) is skipped entirely.  The draw, the finish and whole updates come from tests/_glm_ref.py by import (noise,
draw, finish with D := K D), the predictive noise from the oracle (Philox stream 2, step 0)."""
import math

import numpy as np

import _glm_ref as glm
from oracle import philox

PREDICT_STREAM = 2
EPS = 2e-5      # the project's factor for a float32 dot of <= 256 terms followed by transcendentals


def logits(X, W):
    """l[n, s, k] = sum_d X[n, d] W[s, k, d]."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    W64 = np.asarray(W, np.float32).astype(np.float64)
    return np.einsum("nd,skd->nsk", X64, W64)


def logsumexp(L):
    """Over the last axis, the maximum subtracted."""
    m = L.max(axis=-1, keepdims=True)
    return m[..., 0] + np.log(np.exp(L - m).sum(axis=-1))


def softmax(L):
    e = np.exp(L - L.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def valid_rows(y, K):
    y = np.asarray(y).astype(np.int64)
    return (y >= 0) & (y < K)


def data_pass_from_logits(L, X64, y):
    """ell [S], G [S, K, D] from l [B, S, K] (any float64 logits: the CPU tests perturb them directly)."""
    B, S, K = L.shape
    ok = valid_rows(y, K)
    L, X64, yk = L[ok], X64[ok], np.asarray(y).astype(np.int64)[ok]
    n = np.arange(L.shape[0])
    ell = (L[n, :, yk] - logsumexp(L)).sum(axis=0)
    R = -softmax(L)
    R[n, :, yk] += 1.0
    return ell, np.einsum("nsk,nd->skd", R, X64)


def softmax_data_pass(X, y, W):
    """ell[s] = sum_n (l[n,s,y_n] - lse[n,s]),  G[s,k,:] = sum_n (1[y_n = k] - softmax_k(l[n,s,:])) x_n."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    return data_pass_from_logits(logits(X, W), X64, y)


def ell_bound(X, y, W):
    """sum_n (|l[n,s,y_n]| + |lse[n,s]| + 1) over the rows that count: what 2e-5 multiplies."""
    L = logits(X, W)
    K = L.shape[2]
    ok = valid_rows(y, K)
    L, yk = L[ok], np.asarray(y).astype(np.int64)[ok]
    n = np.arange(L.shape[0])
    return (np.abs(L[n, :, yk]) + np.abs(logsumexp(L)) + 1.0).sum(axis=0)


def log_mean_exp(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(X, W, y=None):
    """dict(prob [B, K][, lpd [B], lpd_sum]) in float64; a row with a label outside [0, K) has lpd = 0."""
    L = logits(X, W)
    B, S, K = L.shape
    out = dict(prob=softmax(L).mean(axis=1))
    if y is not None:
        ok = valid_rows(y, K)
        yk = np.where(ok, np.asarray(y).astype(np.int64), 0)
        lp = L[np.arange(B), :, yk] - logsumexp(L)
        out["lpd"] = np.where(ok, log_mean_exp(lp), 0.0) if B else np.zeros(0)
        out["lpd_sum"] = out["lpd"].sum()
    return out


def predict_bounds(X, W, y=None):
    """Per-entry bounds on |device - reference| (tests/test_softmax_regression_gpu.py's docstring):
    a = max_k sum_d |x_nd w_skd|, per-draw logit error 2e-5 (a + 1)."""
    X64 = np.asarray(X, np.float32).astype(np.float64)
    W64 = np.asarray(W, np.float32).astype(np.float64)
    L = logits(X, W)
    a = np.einsum("nd,skd->nsk", np.abs(X64), np.abs(W64)).max(axis=2)         # [B, S]
    p = softmax(L)
    out = dict(prob=(EPS * (2.0 * p * a[:, :, None] + p)).mean(axis=1))
    if y is not None:
        K = L.shape[2]
        ok = valid_rows(y, K)
        e = 2.0 * EPS * (a + np.abs(logsumexp(L)) + 1.0)
        out["lpd"] = np.where(ok, e.max(axis=1), 0.0) if L.shape[0] else np.zeros(0)
        out["lpd_sum"] = out["lpd"].sum()
    return out


# ---- the guide: tests/_glm_ref.py's at width K D ---------------------------------------------------------------

def init_lam(K, D):
    return glm.init_lam(K * D)


def softmax_step(lam, m1, m2, t, X, y, K, S, seed, n_total, lr, tau=1.0):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as SoftmaxReparamSVI does
    it.  Returns (lam, m1, m2, elbo, grad)."""
    B, D = X.shape
    P = K * D
    eps = glm.noise(P, S, seed, t - 1)
    W = glm.draw(lam, eps)
    ell, G = softmax_data_pass(X, y, W.reshape(S, K, D))
    return glm.finish(lam, m1, m2, t, eps, W, ell, G.reshape(S, P), n_total / B, tau, lr)


def posterior_draws(lam, K, D, S, seed):
    """svi/predict.py's draws for the mean-field guide: W float32 [S, K, D]."""
    P = K * D
    lam = np.asarray(lam, np.float64)
    eps = philox.normal_draws(seed, S, P, stream=PREDICT_STREAM, step=0)
    return (lam[None, :P] + np.exp(lam[P:2 * P])[None, :] * eps).astype(np.float32).reshape(S, K, D)


def ar_design(B, D, K, seed):
    """AR(0.9) features with unit marginal variance, W* = N(0, 1) [K, D], y ~ Categorical(softmax(W* x))."""
    r = np.random.RandomState(seed)
    X = np.empty((B, D))
    X[:, 0] = r.standard_normal(B)
    for d in range(1, D):
        X[:, d] = 0.9 * X[:, d - 1] + math.sqrt(1.0 - 0.81) * r.standard_normal(B)
    p = softmax(X @ r.standard_normal((K, D)).T)
    u = r.uniform(size=B)
    y = (u[:, None] > np.cumsum(p, axis=1)).sum(axis=1).clip(0, K - 1)
    return X.astype(np.float32), y.astype(np.int32)
