"""Float64 numpy restatement of the Beta route (include/bayesic_hip.h: bsc_glm_beta_data_pass, bsc_glm_beta_update,
bsc_beta_predict_pass; svi/glm_beta.py):

    y_n ~ Beta(a, b),  0 < y < 1,  a = m phi,  b = (1 - m) phi,  m = sigmoid(l),  l[n,s] = x_n . w_s + o_n,  phi_s = e^{tau_s}
    ly = log y,  l1y = log1p(-y)
    log p(y | l, phi) = lnGamma(phi) - lnGamma(a) - lnGamma(b) + (a - 1) ly + (b - 1) l1y
    ell[s] = sum_n v_n log p(y_n | l_ns, phi_s)
    r[n,s] = v_n phi_s m (1 - m) [ (ly - l1y) - psi(a) + psi(b) ],   G[s,:] = sum_n r[n,s] x_n
    T[s]   = sum_n v_n phi_s [ psi(phi_s) + m (ly - psi(a)) + (1 - m)(l1y - psi(b)) ]

under w ~ N(0, I / prec), phi ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select.  m and 1 - m are scipy's expit(l) and expit(-l): neither is formed by subtraction.  The prior on
the scalar has the negative binomial's form, so the draws, the finish and the stepper's Adam are tests/_glm_nb_ref.py's
by import (log phi, the precision, in the place of its log-dispersion), the size of the ELBO's terms is
tests/_glm_gamma_ref.py's; the logits come from tests/_glm_obs_ref.py.

The bound quantities are the sums of the sizes of the terms the device forms (csrc/bsc_special_f32.h,
bsc_lgamma_psi_f32: an argument below 8 is shifted up to at least 8, so lnGamma(x) is the difference of a Stirling term
of size S(x) = max(|lnGamma(max(x, 8))|, 17) -- 17 covers (x + n - 1/2) log(x + n) - (x + n) up to x + n = 9 with its
constant -- and log P, which S(x) covers above x = 1 and |log x| below):

    b_ell = sum_n v ( |lnGamma phi| + S(a) + S(b) + |log min(a, 1)| + |log min(b, 1)| + (a + 1)|ly| + (b + 1)|l1y| + 1 )
    b_T   = sum_n v ( phi (|psi phi| + m (|ly| + |psi a|) + (1 - m)(|l1y| + |psi b|)) + 1 )"""
import math

import numpy as np
from scipy.special import digamma, expit, gammaln

import _glm_gamma_ref as gamma
import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

LOG_2PI = nb.LOG_2PI
EPS = 2e-5
TAU_LO, TAU_HI = -2.0, 5.0          # the accuracy envelope (include/bayesic_hip.h)
Y_LO, Y_HI = 1.0e-6, 1.0 - 1.0e-6
_f64 = obs._f64


# ---- inputs shared by tests/test_glm_beta_cpu.py and tests/test_glm_beta_gpu.py ------------------------------------------

def make_inputs(B, D, S, seed, mode="both"):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every fifth
    exactly zero) with tau uniform in the accuracy envelope [-2, 5], its smallest and largest moved to the two ends, and y
    drawn from Beta(5 m, 5 (1 - m)) at the first draw's logit, clipped to [1e-6, 1 - 1e-6]; every seventh row sits at 1e-6
    and every eleventh at 1 - 1e-6.
    Returns (X, y, W, logprec, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o = mode in ("offset", "both")
    m = expit(obs.logits(X, W, o if use_o else None)[:, 0])
    y = rs.beta(5.0 * m, 5.0 * (1.0 - m))
    y[6::7] = Y_LO
    y[3::11] = Y_HI
    y = np.clip(y, Y_LO, Y_HI).astype(np.float32)
    logprec = rs.uniform(TAU_LO, TAU_HI, S).astype(np.float32)
    if S > 1:                                   # both ends of the envelope are in every batch of draws
        logprec[np.argmin(logprec)], logprec[np.argmax(logprec)] = TAU_LO, TAU_HI
    return X, y, W, logprec, (o if use_o else None), (v if mode in ("weights", "both") else None)


def make_extreme_inputs(D, B, flip, S=8):
    """Integer logits of +-80 of which +-75 come from the offset (flip = 1), and +-70 with the offset flipped (flip =
    -1): one-hot X, W = +-5.  tau cycles through {-2, 0, 5} over the draws, y through {1e-6, 1/4, 1/2, 1 - 1e-6} over the
    rows; every row has a weight of 1, 2 or 3.  Returns (X, y, W, logprec, offset, weights)."""
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(D)[None, :])
    W = (5.0 * sign).astype(np.float32)
    logprec = np.array([TAU_LO, 0.0, TAU_HI], np.float32)[np.arange(S) % 3]
    y = np.array([Y_LO, 0.25, 0.5, Y_HI], np.float32)[(np.arange(B) // 2) % 4]
    v = (1.0 + (np.arange(B) % 3)).astype(np.float32)
    o = (flip * 75.0 * sign[0, np.arange(B) % D]).astype(np.float32)
    return X, y, W, logprec, o, v


# ---- the pass -------------------------------------------------------------------------------------------------------

def stirling_size(x):
    """S(x) = max(|lnGamma(max(x, 8))|, 17): the size of the shifted Stirling term behind lnGamma(x)."""
    return np.maximum(np.abs(gammaln(np.maximum(x, 8.0))), 17.0)


def _parts(L, y, logprec, phi=None):
    """What every formula here is made of, float64 [B, S] (phi [1, S], ly and l1y [B, 1]).  ``phi``: the precisions
    themselves, float64 [S], in the place of e^{logprec} (logprec is a float32 operand: e^tau = 2 exactly has no tau)."""
    y64 = _f64(y)[:, None]
    phi = np.exp(_f64(logprec))[None, :] if phi is None else np.asarray(phi, np.float64)[None, :]
    m, m1 = expit(L), expit(-L)
    with np.errstate(invalid="ignore", divide="ignore"):
        ly, l1y = np.log(y64), np.log1p(-y64)
    return phi, m, m1, m * phi, m1 * phi, ly, l1y


def _terms(X, y, W, logprec, offset, weights):
    """Per (row, draw): the terms of ell, their absolute sizes, the residual, the terms of T, their absolute sizes."""
    L = obs.logits(X, W, offset)
    phi, m, m1, a, b, ly, l1y = _parts(L, y, logprec)
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        psa, psb = digamma(a), digamma(b)
        t_ell = np.where(on, vv * (gammaln(phi) - gammaln(a) - gammaln(b) + (a - 1.0) * ly + (b - 1.0) * l1y), 0.0)
        a_ell = np.where(on, vv * (np.abs(gammaln(phi)) + stirling_size(a) + stirling_size(b)
                                   + np.abs(np.log(np.minimum(a, 1.0))) + np.abs(np.log(np.minimum(b, 1.0)))
                                   + (a + 1.0) * np.abs(ly) + (b + 1.0) * np.abs(l1y) + 1.0), 0.0)
        r = np.where(on, vv * phi * m * m1 * ((ly - l1y) - psa + psb), 0.0)
        t_T = np.where(on, vv * phi * (digamma(phi) + m * (ly - psa) + m1 * (l1y - psb)), 0.0)
        a_T = np.where(on, vv * (phi * (np.abs(digamma(phi)) + m * (np.abs(ly) + np.abs(psa))
                                        + m1 * (np.abs(l1y) + np.abs(psb))) + 1.0), 0.0)
    return t_ell, a_ell, r, t_T, a_T


def data_pass(X, y, W, logprec, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, t_T, _ = _terms(X, y, W, logprec, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, logprec, offset=None, weights=None):
    """(b_ell [S], b_T [S]) of the module docstring: what the device's errors of ell and T are measured against (each
    times 2e-5), rows of weight 0 left out."""
    _, a_ell, _, _, a_T = _terms(X, y, W, logprec, offset, weights)
    return a_ell.sum(axis=0), a_T.sum(axis=0)


def row_logpdf(L, y, logprec, phi=None):
    """log p(y_n | l_ns, phi_s), the full density: [B, S] (``phi``: as in _parts)."""
    phi, _, _, a, b, ly, l1y = _parts(L, y, logprec, phi)
    return gammaln(phi) - gammaln(a) - gammaln(b) + (a - 1.0) * ly + (b - 1.0) * l1y


def lgamma_psi_f32(x):
    """csrc/bsc_special_f32.h's bsc_lgamma_psi_f32 in plain float32 numpy: the argument shifted up to at least 8 by one
    product of at most eight factors carried with its derivative, three asymptotic terms there."""
    f = np.float32
    x = np.asarray(x, f)
    n = (f(8) - x).astype(f)
    P, dP, zz = np.ones_like(x), np.zeros_like(x), x.copy()
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(8):
            take = f(i) < n
            fac = (x + f(i)).astype(f)
            dP = np.where(take, (dP * fac + P).astype(f), dP)
            P = np.where(take, (P * fac).astype(f), P)
            zz = np.where(take, (fac + f(1)).astype(f), zz)
        lz = np.log(zz).astype(f)
        inv = (f(1) / zz).astype(f)
        inv2 = (inv * inv).astype(f)
        st = (((zz - f(0.5)) * lz - zz).astype(f) + f(0.91893853320467274)
              + inv * (f(1 / 12) - inv2 * (f(1 / 360) - inv2 * f(1 / 1260)))).astype(f)
        asym = (lz - f(0.5) * inv - inv2 * (f(1 / 12) - inv2 * (f(1 / 120) - inv2 * f(1 / 252)))).astype(f)
        return (st - np.log(P).astype(f)).astype(f), (asym - (dP * (f(1) / P).astype(f)).astype(f)).astype(f)


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def link_f32(l, y, tau):
    """The kernel's link (csrc/bsc_glm_pass.h, GLM_BETA) in plain float32: l [B, S], y [B], tau [S] float32; lnGamma(phi)
    and psi(phi) are float64 values rounded, as on the device.  Returns the per-(row, draw) terms of ell, the residual
    and the terms of T without the weight, float32 [B, S]."""
    f = np.float32
    one = f(1)
    phi = np.exp(tau).astype(f)[None, :]
    lg0 = gammaln(phi.astype(np.float64)).astype(f)
    ps0 = digamma(phi.astype(np.float64)).astype(f)
    yq = y[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-np.abs(l)).astype(f)
        r = (one / (one + e)).astype(f)
        er = (e * r).astype(f)
        pos = l >= 0
        m, m1 = np.where(pos, r, er), np.where(pos, er, r)
        ly = np.log(yq).astype(f)
        w = (one - yq).astype(f)
        is1 = w == one
        ratio = (yq * (one / np.where(is1, one, (one - w).astype(f))).astype(f)).astype(f)
        l1y = ((np.log(w).astype(f) * ratio).astype(f) + np.where(is1, -yq, f(0))).astype(f)
        a, b = (m * phi).astype(f), (m1 * phi).astype(f)
        lga, psa = lgamma_psi_f32(a)
        lgb, psb = lgamma_psi_f32(b)
        t_ell = (((lg0 - lga).astype(f) - lgb).astype(f)
                 + (((a - one).astype(f) * ly).astype(f) + ((b - one).astype(f) * l1y).astype(f)).astype(f)).astype(f)
        inner = ((m * (ly - psa).astype(f)).astype(f) + (m1 * (l1y - psb).astype(f)).astype(f)).astype(f)
        t_T = (phi * (ps0 + inner).astype(f)).astype(f)
        res = ((phi * (er * r).astype(f)).astype(f) * (((ly - l1y).astype(f) - psa).astype(f) + psb).astype(f)).astype(f)
    return t_ell, res, t_T


def data_pass_f32(X, y, W, logprec, offset=None, weights=None):
    """The kernel's formulas evaluated plainly in float32.  The sums follow the pass's design, float32 partials finished
    in float64: F32_BLOCK rows are added in float32 (the largest partial of a pass that runs one tile per wave), the
    partials in float64 (tests/_glm_gamma_ref.data_pass_f32 says why)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, logprec))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    keep = v > 0
    X, y, o, v = X[keep], y[keep], o[keep], v[keep]
    l = ((X[:, None, :] * W[None, :, :]).sum(axis=2, dtype=f) + o[:, None]).astype(f)
    t_ell, res, t_T = link_f32(l, y, tau)
    vv = v[:, None]
    ell, G, T = np.zeros(S), np.zeros((S, D)), np.zeros(S)
    for k in range(0, X.shape[0], F32_BLOCK):
        s = slice(k, k + F32_BLOCK)
        ell += (vv[s] * t_ell[s]).astype(f).sum(axis=0, dtype=f).astype(np.float64)
        T += (vv[s] * t_T[s]).astype(f).sum(axis=0, dtype=f).astype(np.float64)
        G += ((vv[s] * res[s]).astype(f).T @ X[s]).astype(np.float64)
    return ell, G, T


# ---- draws and the finish: the negative binomial's (the scalar's prior has the same form) ---------------------------------

init_lam = nb.init_lam              # m = 0 (tau = 0), rho = log 0.1
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1]
draw = nb.draw                      # (W [S, D] float32, logprec [S] float32)
log_prior_tau = nb.log_prior_tau
elbo_and_grad = nb.elbo_and_grad    # (lam, eps, W, logprec, ell, G, T, scale, prec, a0, b0)
update = nb.finish                  # bsc_glm_beta_update from given statistics: (lam', m1', m2', elbo, grad)
elbo_terms_size = gamma.elbo_terms_size     # (W, logprec, b_ell, scale, prec, a0, b0, rho): the same prior, the same terms


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as BetaReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logprec = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, logprec, offset, weights)
    return update(lam, m1, m2, t, eps, W, logprec, ell, G, T, n_total / B, prec, a0, b0, lr)


RECOVERY = dict(seed=5, rows=3000, heldout=500, steps=300, lr=0.05, S=8, driver_seed=11)


def recovery_data(seed, B=RECOVERY["rows"] + RECOVERY["heldout"], D=8, phi=20.0):
    """Simulated rows at a true precision ``phi``: an intercept column and D - 1 features N(0, 1) / sqrt(D), w_true ~
    0.8 N; y clipped to [1e-6, 1 - 1e-6].  The first RECOVERY["rows"] are fitted, the rest held out.  Returns (X, y,
    w_true).  tests/test_glm_beta_cpu.py runs the reference alone on them, tests/test_glm_beta_gpu.py the driver."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    X[:, 0] = 1.0
    w_true = 0.8 * rs.standard_normal(D)
    m = expit(X.astype(np.float64) @ w_true)
    y = np.clip(rs.beta(m * phi, (1.0 - m) * phi), Y_LO, Y_HI).astype(np.float32)
    return X, y, w_true



# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], logprec float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def predict(X, W, logprec, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    phi = np.exp(_f64(logprec))[None, :]
    mu = expit(L)
    v = mu * expit(-L) / (1.0 + phi)
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        lp = row_logpdf(L, y, logprec)
        m = lp.max(axis=1, keepdims=True)
        out["lpd"] = m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, W, logprec, y=None, offset=None, weights=None):
    """tests/_glm_nb_ref.predict_bounds' construction for this family.  With a_ns = sum_d |x_nd w_sd| + |o_n| the size of
    the logit's float32 terms and EPS = 2e-5:  mu = m, dm/dl = m (1 - m): e_mu = EPS (m (1 - m) a + m), the logistic
    family's;  v = m (1 - m) / (1 + phi), |dv/dl| = v |1 - 2 m| <= v: e_v = EPS (v a + v), the second term also covering
    the float32 1 / (1 + phi);  log p: EPS times the sizes of its terms (the pass's ell bound per row), maximum over the
    draws.  (The logit's own error enters log p through phi m (1 - m) [(ly - l1y) - psi(a) + psi(b)]: phi m (1 - m) is
    below both a and b, a |ly| + b |l1y| is in the bound, and x |psi(x)| is below 1 + |log x| + x |log x|, which the
    Stirling size and |log min(x, 1)| cover.)"""
    X64, W64 = _f64(X), _f64(W)
    L = obs.logits(X, W, offset)
    a_l = np.abs(X64) @ np.abs(W64).T
    if offset is not None:
        a_l = a_l + np.abs(_f64(offset))[:, None]
    phi = np.exp(_f64(logprec))[None, :]
    mu = expit(L)
    mm = mu * expit(-L)
    v = mm / (1.0 + phi)
    e_mu = EPS * (mm * a_l + mu)
    e_v = EPS * (v * a_l + v)
    mean = mu.mean(axis=1)
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        _, m, m1, a, b, ly, l1y = _parts(L, y, logprec)
        e = EPS * (np.abs(gammaln(phi)) + stirling_size(a) + stirling_size(b) + np.abs(np.log(np.minimum(a, 1.0)))
                   + np.abs(np.log(np.minimum(b, 1.0))) + (a + 1.0) * np.abs(ly) + (b + 1.0) * np.abs(l1y) + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
