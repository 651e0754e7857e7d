"""Float64 numpy restatement of the ordinal (cumulative-logit) route (include/bayesic_hip.h: bsc_glm_ordinal_data_pass,
bsc_ordinal_predict_pass; svi/glm_ordinal.py):

    y_n in {0 .. K-1},  eta[n,s] = x_n . w_s + o_n,  c_0 < .. < c_{K-2},  c_{-1} = -inf,  c_{K-1} = +inf
    P(y = k) = sigmoid(c_k - eta) - sigmoid(c_{k-1} - eta)
    theta_0 = c_0,  theta_j = log(c_j - c_{j-1});  z = [w (D) | theta (K - 1)] ~ N(0, I / prec),  P = D + K - 1
    ell[s] = sum_n v_n log P(y_n),   G[s, :D] = sum_n v_n (d log P / d eta) x_n,   G[s, D + i] = d ell[s] / d theta_i

The cutpoints are part of the INPUT as the interface defines it: the float32 roundings of the float64 cumulative sum of
the float32 theta (``cutpoints``).  From there on this file is independent of the device's formulas where it can be: with
a = c_{y-1} - eta, b = c_y - eta the probability is the plain difference p = sigmoid(b) - sigmoid(a) (taken on the side
where both sigmoids are below 1/2 of their mirror images, i.e. as sigmoid(-a) - sigmoid(-b) when a > 0) and its
derivatives are s'(b) / p and -s'(a) / p with s' = s (1 - s), wherever that difference is well conditioned
((s_b + s_a) / p < 1e4: float64 then leaves 1e-12); only elsewhere -- a narrow class far out in a tail -- the product form
log p = log s(b) + log s(-a) + log(-expm1(-g)), g = c_y - c_{y-1}, and its derivatives take over.  The chain rule to theta
is d/d theta_0 = sum_j H_j, d/d theta_i = e^{theta_i} sum_{j >= i} H_j with H_j = d ell / d c_j.

Rows of weight 0 and rows whose label is outside [0, K) are dropped by a select, whatever they hold.  Draws, finish and
Adam are tests/_glm_ref.py's and tests/_glm_full_ref.py's at width P; the logits come from tests/_glm_obs_ref.py.

The bound quantities (``bounds``, ``predict_bounds``) are the sums of the absolute sizes of the terms, with the
conditioning of a and b on their rounded inputs: each is formed in float32 from a rounded cutpoint and a linear predictor
whose float32 terms have the size A = sum_d |x_d w_d| + |o|, so its absolute error is a multiple of eps times
ca = |c_{y-1}| + A + |a| (cb alike), and that costs |d log p / d a| ca of log p.  With U = [y < K-1], L = [y > 0], sp the
softplus, s the sigmoid, s' its derivative and q = U L / expm1(g), per kept (row, draw):
    ell:        U sp(-b) + L sp(a) + U L |log(-expm1(-g))| + U s(-b) cb + L s(a) ca
    r:          L s(a) + U s(-b) + L s'(a) ca + U s'(b) cb
    dc_y:       U (s(-b) + s'(b) cb) + q          dc_{y-1}:  L (s(a) + s'(a) ca) + q
and the bound of d ell / d theta_i is the chain rule applied to the bounds of the H_j.  A device result is held to
EPS = 2e-5 times these, a plain float32 evaluation to EPS / 20 (tests/test_glm_ordinal_cpu.py), as
tests/_glm_weibull_ref.py holds its model."""
import math

import numpy as np

import _glm_full_ref as full
import _glm_obs_ref as obs
import _glm_ref as mf
from oracle import philox

LOG_2PI = mf.LOG_2PI
EPS = 2e-5
GAP_LO, GAP_HI = -3.0, 1.5       # the accuracy envelope of the log-gaps (include/bayesic_hip.h): gaps 0.05 .. 4.5
ETA_MAX = 30.0
WELL = 1.0e4                     # (s_b + s_a) / p below this: the plain difference is used
BAD_LABELS = (-1, None, 2 ** 31 - 1)   # what a dropped row holds in turn (None: K)
_f64 = obs._f64


def cutpoints(theta):
    """c [.., K - 1] as the pass defines them: float32(cumsum in float64 of [theta_0, e^{theta_1}, ..]) of the float32
    theta, returned as float64."""
    th = _f64(np.asarray(theta, np.float32))
    steps = np.concatenate([th[..., :1], np.exp(th[..., 1:])], axis=-1)
    return _f64(np.cumsum(steps, axis=-1).astype(np.float32))


def split(Z, D, K):
    """(W [S, D], theta [S, K - 1]) of draws Z [S, >= D + K - 1]."""
    Z = np.asarray(Z, np.float32)
    return Z[:, :D], Z[:, D:D + K - 1]


# ---- inputs shared by tests/test_glm_ordinal_cpu.py and tests/test_glm_ordinal_gpu.py ---------------------------------

def make_inputs(B, D, S, K, seed, mode="both"):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3)) with, per draw,
    theta_0 ~ N(-1, 0.5) and log-gaps spread over the accuracy envelope [-3, 1.5].  Labels are drawn from the model at
    the first draw's cutpoints widened to unit gaps (so that no level is rare), and the first K kept rows hold
    0 .. K-1: every level occurs.  With weights, every eleventh row has weight 0 (at most 10 % of the rows) and holds
    -1, K and 2^31 - 1 in turn: labels a kept row must not hold.
    Returns (X, y int32, Z float32 [S, D + K - 1], offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[5::11] = 0.0
    theta = np.empty((S, K - 1))
    theta[:, 0] = -1.0 + 0.5 * rs.standard_normal(S)
    for s in range(S):
        theta[s, 1:] = np.linspace(GAP_LO, GAP_HI, K - 2)[rs.permutation(K - 2)] if K > 3 else \
            rs.uniform(GAP_LO, GAP_HI, K - 2)
    Z = np.concatenate([W, theta.astype(np.float32)], axis=1)
    use_o, use_v = mode in ("offset", "both"), mode in ("weights", "both")
    eta = obs.logits(X, W, o if use_o else None)[:, 0]
    c_gen = -1.0 + np.arange(K - 1) - 0.5 * (K - 2)
    u = rs.uniform(size=B)
    cum = 1.0 / (1.0 + np.exp(-(c_gen[None, :] - eta[:, None])))
    y = (u[:, None] > cum).sum(axis=1).astype(np.int32)
    keep = (v > 0) if use_v else np.ones(B, bool)
    y[np.flatnonzero(keep)[:K]] = np.arange(K)
    if use_v:
        dead = np.flatnonzero(v == 0)
        for i, bad in enumerate(BAD_LABELS):
            y[dead[i::3]] = K if bad is None else bad
    return X, y, Z, (o if use_o else None), (v if use_v else None)


W_TRUE = np.array([0.9, -0.7, 0.5, 0.4, -0.3, 0.6, -0.5, 0.2])
C_TRUE = np.array([-1.5, -0.5, 0.5, 1.5])       # K = 5, separated cutpoints


def simulate(B, seed):
    """(X [B, 8], y int32 [B]) from the cumulative-logit model at W_TRUE and C_TRUE (K = 5), X ~ 1.5 N(0, I)."""
    rs = np.random.RandomState(seed)
    X = (1.5 * rs.standard_normal((B, len(W_TRUE)))).astype(np.float32)
    eta = X.astype(np.float64) @ W_TRUE
    cum = 1.0 / (1.0 + np.exp(-(C_TRUE[None, :] - eta[:, None])))
    return X, (rs.uniform(size=B)[:, None] > cum).sum(axis=1).astype(np.int32)


def frequency_baseline(y_train, y_test, K):
    """Mean log-likelihood of y_test under the class frequencies of y_train: what a model without X achieves."""
    freq = np.bincount(y_train, minlength=K) / float(len(y_train))
    return float(np.log(freq[y_test]).mean())


def fit(X, y, K, S, seed, steps, lr, prec=1.0):
    """The reference driver alone, full batch, from the default start: (lam, [elbo of every step])."""
    lam = init_lam(X.shape[1] + K - 1)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    elbos = []
    for t in range(1, steps + 1):
        lam, m1, m2, elbo, _ = step(lam, m1, m2, t, X, y, K, S, seed, float(X.shape[0]), lr, prec)
        elbos.append(elbo)
    return lam, elbos


# ---- the pass -------------------------------------------------------------------------------------------------------

def logit_size(X, W, offset):
    """A[n,s] = sum_d |x_nd w_sd| + |o_n|: the size of the linear predictor's float32 terms."""
    a = np.abs(_f64(X)) @ np.abs(_f64(W)).T
    return a if offset is None else a + np.abs(_f64(offset))[:, None]


def _sig(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def _sp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _terms(X, y, Z, K, offset, weights):
    """Per (row, draw), zero on a dropped row: log p, d log p / d eta, d log p / d c_y, d log p / d c_{y-1}, and the four
    bound quantities of the module docstring; also keep [B] and the clamped labels [B]."""
    B, D = X.shape
    W, theta = split(Z, D, K)
    S = W.shape[0]
    eta = obs.logits(X, W, offset)
    A = logit_size(X, W, offset)
    c = cutpoints(theta)
    cpad = np.concatenate([np.full((S, 1), -np.inf), c, np.full((S, 1), np.inf)], axis=1)     # c_{k-1} at [k], c_k at [k+1]
    y = np.asarray(y).astype(np.int64)
    v = np.ones(B) if weights is None else _f64(weights)
    keep = (v > 0) & (y >= 0) & (y < K)
    yq = np.where(keep, y, 0)
    lo, hi = cpad[:, yq].T, cpad[:, yq + 1].T                # [B, S]
    U, L = (yq < K - 1)[:, None], (yq > 0)[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a, b = lo - eta, hi - eta
        # the plain difference, on the side where the sigmoids are small
        flip = np.where(np.isfinite(a), a, b) > 0
        sb, sa = _sig(np.where(flip, -a, b)), _sig(np.where(flip, -b, a))      # p = sb - sa either way
        p = sb - sa
        well = (sb + sa) < WELL * p
        dsb, dsa = _sig(b) * _sig(-b), _sig(a) * _sig(-a)    # s'(+-inf) = 0
        g = np.where(U & L, hi - lo, 1.0)
        lg = np.where(U & L, np.log(-np.expm1(-g)), 0.0)
        q = np.where(U & L, 1.0 / np.expm1(g), 0.0)
        spb, spa = np.where(U, _sp(-b), 0.0), np.where(L, _sp(a), 0.0)
        s_mb, s_a = np.where(U, _sig(-b), 0.0), np.where(L, _sig(a), 0.0)
        logp = np.where(well, np.log(np.where(well, p, 1.0)), lg - spb - spa)
        pw = np.where(well, p, 1.0)
        r = np.where(well, (dsa - dsb) / pw, s_a - s_mb)
        hu = np.where(well, dsb / pw, s_mb + q)
        hl = np.where(well, -dsa / pw, -(s_a + q))
        ca = np.where(L, np.abs(np.where(L, lo, 0.0)) + A + np.abs(np.where(L, a, 0.0)), 0.0)
        cb = np.where(U, np.abs(np.where(U, hi, 0.0)) + A + np.abs(np.where(U, b, 0.0)), 0.0)
        a_ell = spb + spa + np.abs(lg) + s_mb * cb + s_a * ca
        a_r = s_a + s_mb + np.where(L, dsa, 0.0) * ca + np.where(U, dsb, 0.0) * cb
        a_hu = s_mb + np.where(U, dsb, 0.0) * cb + q
        a_hl = s_a + np.where(L, dsa, 0.0) * ca + q
    vv = np.where(keep, v, 0.0)[:, None]
    k2 = keep[:, None]
    z = lambda t: np.where(k2, vv * t, 0.0)
    return dict(logp=z(logp), r=z(r), hu=z(hu), hl=z(hl), a_ell=z(a_ell), a_r=z(a_r), a_hu=z(a_hu), a_hl=z(a_hl),
                keep=keep, yq=yq, theta=_f64(theta), raw_logp=np.where(k2, logp, 0.0), raw_a_ell=np.where(k2, a_ell, 0.0))


def _chain(hu, hl, keep, yq, theta, K):
    """[S, K - 1]: H_j[s] = sum_n [y = j] hu + [y = j + 1] hl, then d/d theta_0 = sum_j H_j and d/d theta_i = e^{theta_i}
    sum_{j >= i} H_j."""
    S = theta.shape[0]
    H = np.zeros((S, K - 1))
    for j in range(K - 1):
        H[:, j] = hu[keep & (yq == j)].sum(axis=0) + hl[keep & (yq == j + 1)].sum(axis=0)
    tail = np.cumsum(H[:, ::-1], axis=1)[:, ::-1]            # sum_{j >= i} H_j
    scale = np.concatenate([np.ones((S, 1)), np.exp(theta[:, 1:])], axis=1)
    return scale * tail


def data_pass(X, y, Z, K, offset=None, weights=None):
    """(ell [S], G [S, P]): float32 operands, float64 arithmetic."""
    t = _terms(X, y, Z, K, offset, weights)
    Gw = t["r"].T @ _f64(X)
    return t["logp"].sum(axis=0), np.concatenate([Gw, _chain(t["hu"], t["hl"], t["keep"], t["yq"], t["theta"], K)], axis=1)


def bounds(X, y, Z, K, offset=None, weights=None):
    """(b_ell [S], b_G [S, P]): what the errors are measured against (module docstring), dropped rows left out."""
    t = _terms(X, y, Z, K, offset, weights)
    bw = t["a_r"].T @ np.abs(_f64(X))
    return t["a_ell"].sum(axis=0), np.concatenate(
        [bw, _chain(t["a_hu"], t["a_hl"], t["keep"], t["yq"], t["theta"], K)], axis=1)


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def data_pass_f32(X, y, Z, K, offset=None, weights=None):
    """The pass's own forms (include/bayesic_hip.h) evaluated plainly in float32 (every array below is float32), with
    the per-(draw, class) constants made in float64 and rounded, as the interface says.  The sums follow the pass's
    design: F32_BLOCK rows are added one after the other in float32, the partials in float64; the chain rule to theta is
    applied in float64 (tests/_glm_weibull_ref.data_pass_f32 says why)."""
    f = np.float32
    X = np.asarray(X, f)
    B, D = X.shape
    W, theta = split(Z, D, K)
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    y = np.asarray(y).astype(np.int64)
    keep = (v > 0) & (y >= 0) & (y < K)
    yq = np.where(keep, y, 0)
    c = cutpoints(theta).astype(f)                                               # [S, K - 1]
    lo_t = np.concatenate([c[:, :1], c], axis=1)                                 # class k: c_{k-1} (class 0: c_0)
    hi_t = np.concatenate([c, c[:, -1:]], axis=1)                                # class k: c_k (class K-1: c_{K-2})
    mid = np.zeros(K, bool)
    mid[1:K - 1] = True
    g = (hi_t - lo_t).astype(np.float64)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        lg_t = np.where(mid[None, :], np.log(-np.expm1(-np.where(mid[None, :], g, 1.0))), 0.0).astype(f)
        ie_t = np.where(mid[None, :], 1.0 / np.expm1(np.where(mid[None, :], g, 1.0)), 0.0).astype(f)
    one, zero = f(1.0), f(0.0)

    def logistic(x):
        e = np.exp(-np.abs(x))
        t = one + e
        return np.maximum(x, zero) + np.log1p(e), np.where(x >= 0, one, e) / t

    with np.errstate(over="ignore", invalid="ignore"):
        l = np.where(keep[:, None], X @ W.T + o[:, None], zero)
        vq = np.where(keep, v, zero)[:, None]
        Uf = np.where(yq < K - 1, one, zero)[:, None]
        Lf = np.where(yq > 0, one, zero)[:, None]
        sp_b, sg_b = logistic(l - hi_t[:, yq].T)
        sp_a, sg_a = logistic(lo_t[:, yq].T - l)
        t_ell = vq * (lg_t[:, yq].T - (Uf * sp_b + Lf * sp_a))
        hu = vq * (Uf * (sg_b + ie_t[:, yq].T))
        hl = -vq * (Lf * (sg_a + ie_t[:, yq].T))
        r = vq * (Lf * sg_a - Uf * sg_b)
    assert t_ell.dtype == f and r.dtype == f and hu.dtype == f and hl.dtype == f and l.dtype == f
    ell, G, H = np.zeros(S), np.zeros((S, D)), np.zeros((S, K - 1))
    for b0 in range(0, B, F32_BLOCK):
        sl = slice(b0, b0 + F32_BLOCK)
        ell += np.cumsum(t_ell[sl], axis=0, dtype=f)[-1]
        G += np.cumsum(r[sl, :, None] * X[sl, None, :], axis=0, dtype=f)[-1]
        for j in range(K - 1):
            h = np.where((yq[sl] == j)[:, None], hu[sl], np.where((yq[sl] == j + 1)[:, None], hl[sl], zero))
            H[:, j] += np.cumsum(h, axis=0, dtype=f)[-1]
    tail = np.cumsum(H[:, ::-1], axis=1)[:, ::-1]
    scale = np.concatenate([np.ones((S, 1)), np.exp(_f64(theta)[:, 1:])], axis=1)
    return ell, np.concatenate([G, scale * tail], axis=1)


# ---- draws and the finish: tests/_glm_ref.py's and tests/_glm_full_ref.py's at width P ------------------------------------

def init_lam(P, covariance="diag"):
    return full.init_lam(P) if covariance == "full" else mf.init_lam(P)


def noise(P, S, seed, step):
    return mf.noise(P, S, seed, step)


def draw(lam, eps, covariance="diag"):
    """Z [S, P] float32."""
    return full.draw(lam, eps) if covariance == "full" else mf.draw(lam, eps)


def update(lam, m1, m2, t, eps, Z, ell, G, scale, prec, lr, covariance="diag"):
    """bsc_glm_update / bsc_glm_fullrank_update at D := P from given statistics: (lam', m1', m2', elbo, grad)."""
    fin = full.finish if covariance == "full" else mf.finish
    return fin(lam, m1, m2, t, eps, Z, ell, G, scale, prec, lr)


def step(lam, m1, m2, t, X, y, K, S, seed, n_total, lr, prec=1.0, offset=None, weights=None, covariance="diag"):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as OrdinalReparamSVI does it."""
    B, D = X.shape
    eps = noise(D + K - 1, S, seed, t - 1)
    Z = draw(lam, eps, covariance)
    ell, G = data_pass(X, y, Z, K, offset, weights)
    return update(lam, m1, m2, t, eps, Z, ell, G, n_total / B, prec, lr, covariance)


def elbo_terms_size(Z, ell_bound, scale, prec, rho):
    """The sum of the absolute values of the ELBO's terms, from reference quantities alone (tests/_glm_gamma_ref.py)."""
    z = np.asarray(Z, np.float64)
    P = z.shape[1]
    per_draw = scale * ell_bound + 0.5 * prec * (z * z).sum(axis=1)
    return per_draw.mean() + abs(0.5 * P * math.log(prec / (2.0 * math.pi))) + np.abs(rho).sum() \
        + 0.5 * P * (1.0 + LOG_2PI)


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, P, S, seed, covariance="diag"):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, P].  Returns Z float32 [S, P]."""
    return draw(lam, philox.normal_draws(seed, S, P, stream=2, step=0), covariance)


def class_probs(X, Z, K, offset=None):
    """P(y = k | eta[n,s], c_s): [B, S, K], and the cumulative sigmoids' conditioning [B, S, K] (predict_bounds)."""
    D = X.shape[1]
    W, theta = split(Z, D, K)
    eta = obs.logits(X, W, offset)
    A = logit_size(X, W, offset)
    c = cutpoints(theta)                                               # [S, K - 1]
    x = c[None, :, :] - eta[:, :, None]                                # [B, S, K - 1]
    cum = _sig(x)
    one, zero = np.ones(eta.shape + (1,)), np.zeros(eta.shape + (1,))
    cpad = np.concatenate([zero, cum, one], axis=2)
    # |d cum_k| <= s'(x) (|c_k| + A + |x|) eps, and the difference rounds at the size of its two terms
    e = cum * (1.0 - cum) * (np.abs(c)[None, :, :] + A[:, :, None] + np.abs(x)) + cum
    epad = np.concatenate([zero, e, one], axis=2)
    return cpad[:, :, 1:] - cpad[:, :, :-1], epad[:, :, 1:] + epad[:, :, :-1]


def _lse_mean(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(X, Z, K, y=None, offset=None, weights=None):
    """prob [B, K] and, with y, lpd (0 on a row whose label is outside [0, K)) and lpd_sum (such rows left out; weighted
    with weights, rows of weight 0 dropped)."""
    out = dict(prob=class_probs(X, Z, K, offset)[0].mean(axis=1))
    if y is not None:
        t = _terms(X, y, Z, K, offset, None)
        out["lpd"] = np.where(t["keep"], _lse_mean(t["raw_logp"]), 0.0)
        w = np.ones(X.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, Z, K, y=None, offset=None, weights=None):
    """prob: EPS times the draw average of the conditioning of its two cumulative sigmoids (class_probs);  log p: EPS
    times the pass's per-row ell quantity (module docstring), maximum over the draws, as tests/_glm_weibull_ref.py."""
    out = dict(prob=EPS * class_probs(X, Z, K, offset)[1].mean(axis=1))
    if y is not None:
        t = _terms(X, y, Z, K, offset, None)
        out["lpd"] = EPS * (t["raw_a_ell"] + 1.0).max(axis=1) * t["keep"]
        w = np.ones(X.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
