"""Float64 numpy restatement of the zero-inflated Poisson route (include/bayesic_hip.h: bsc_glm_zip_data_pass,
bsc_glm_zip_update, bsc_zip_predict_pass; svi/glm_zip.py), with the structure of tests/_glm_nb_ref.py:

    y_n ~ ZIP(pi, mu_n),  mu = e^l,  l[n,s] = x_n . w_s + o_n,  omega_s = e^{tau_s},  pi_s = sigmoid(tau_s),
    L1_s = log1p(omega_s) = softplus(tau_s),  u = tau_s + mu
                 y == 0                                            y > 0
    log p        log(omega + e^{-mu}) - L1                         y l - mu - L1        (-lnGamma(y + 1): predictive only)
    d / d l      -mu sigmoid(-u)                                   y - mu
    d / d tau    sigmoid(u) (1 - pi) (1 - e^{-mu})                 -pi
    ell[s] = sum_n v_n log p,   r[n,s] = v_n d / d l,   G[s,:] = sum_n r[n,s] x_n,   T[s] = sum_n v_n d / d tau

under w ~ N(0, I / prec), omega ~ Gamma(a0, b0); z = [w (D) | tau], lam = [m (P) | rho (P)], P = D + 1.  Rows of weight 0
are dropped by a select, whatever they hold.  The prior on e^tau has the negative binomial's form, so the draws, the
finish and the stepper's Adam are tests/_glm_nb_ref.py's by import (the log odds in the place of log phi); the logits
come from tests/_glm_obs_ref.py.

The bound quantities are per row, v times the magnitudes of the terms added, plus 1 (tests/_glm_nb_ref.bounds'
construction):
    ell:  |tau| + mu + L1 + |y l| + 1
    T:    |d / d tau| + pi + 1
and G as tests/_glm_weibull_interval_ref.py bounds it, the magnitudes of the residual's terms with its conditioning on
the rounded logit, whose float32 terms have the size a = sum_d |x_d w_d| + |o|: with r = sigmoid(-u) on a zero row and
1 on a positive one, d (mu r) / d l = mu r - [y == 0] mu^2 r (1 - r), so
    r:    y + (1 + a) mu r + [y == 0] a mu^2 r (1 - r),      b_G[s,d] = sum_n v_n (that) |x_nd|.
A device result is held to EPS = 2e-5 times these, a plain float32 replay of the device's forms to 1e-6 times these
(tests/test_glm_zip_cpu.py)."""
import math

import numpy as np
from scipy.special import expit, gammaln

import _glm_nb_ref as nb
import _glm_obs_ref as obs
from oracle import philox

LOG_2PI = nb.LOG_2PI
EPS = 2e-5
TAU_LO, TAU_HI = -8.0, 8.0
_f64 = obs._f64


# ---- inputs shared by tests/test_glm_zip_cpu.py and tests/test_glm_zip_gpu.py -------------------------------------------

def make_inputs(B, D, S, seed, mode="both", zeros=None):
    """tests/test_glm_obs_gpu.py's recipe (X ~ N / sqrt(D), W ~ 0.6 N, offsets N(0, 1), weights U(0, 3) with every fifth
    exactly zero) with tau uniform in [-8, 8] and counts drawn at the first draw's logit with a structural-zero share of
    0.3, which leaves about half of the rows zero; every seventh positive row is replaced by a count from [100, 3000).
    With an offset, every third zero row is pushed by it to mu in [1e-3, 50] (log-uniform) at the first draw.
    ``zeros``: 1.0 makes every row zero, 0.0 every row positive (zeros become ones).  With weights, the rows of weight 0
    hold NaN, infinity and a negative value in turn.
    Returns (X, y, W, logodds, offset or None, weights or None)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o, use_v = mode in ("offset", "both"), mode in ("weights", "both")
    tau = rs.uniform(TAU_LO, TAU_HI, S).astype(np.float32)
    L0 = obs.logits(X, W[:1], o if use_o else None)[:, 0]
    y = rs.poisson(np.exp(L0)).astype(np.float32)
    y[rs.uniform(size=B) < 0.3] = 0.0
    big = rs.randint(100, 3000, size=B).astype(np.float32)
    pos = np.flatnonzero(y > 0)
    y[pos[6::7]] = big[pos[6::7]]
    target = np.exp(rs.uniform(math.log(1e-3), math.log(50.0), B))
    if zeros == 1.0:
        y[:] = 0.0
    elif zeros == 0.0:
        y[y == 0] = 1.0
    if use_o:
        zr = np.flatnonzero(y == 0)[::3]
        o[zr] = (np.log(target[zr]) - (L0[zr] - _f64(o[zr]))).astype(np.float32)
    if use_v:
        dead = np.flatnonzero(v == 0)
        y[dead[0::3]] = np.nan
        y[dead[1::3]] = np.inf
        y[dead[2::3]] = -3.0
    return X, y, W, tau, (o if use_o else None), (v if use_v else None)


# The parity cases of tests/test_glm_zip_gpu.py, which tests/test_glm_zip_cpu.py replays in float32: (B, D, S, mode, ldx or
# None, the vectors one float off 16-byte alignment, zeros).  (1003, 12) and (517, 200) reach the 8-row kernel, narrow and
# ragged, (1003, 256) with a vector off alignment the 8-row D == 256 kernel, (1029, 256) aligned the 16-row MFMA kernel
# with a ragged last tile; S = 11 is two launches, the second with dead draw slots.
PARITY_CASES = [
    (1003, 12, 8, "both", 16, (), None), (1003, 12, 3, "none", None, (), None), (1003, 12, 11, "weights", None, (), 1.0),
    (1003, 12, 8, "offset", None, (), 0.0), (517, 200, 11, "offset", None, (), None), (517, 200, 3, "both", 208, (), None),
    (1003, 256, 8, "both", None, ("y",), None), (1003, 256, 11, "none", None, ("y",), None),
    (1003, 256, 3, "both", None, ("o",), None), (1029, 256, 8, "both", None, (), None),
    (1029, 256, 11, "weights", 260, (), None), (1029, 256, 3, "offset", None, (), None),
    (261, 256, 8, "both", None, (), 1.0), (261, 256, 8, "both", None, (), 0.0)]
# (The all-zero batch on the MFMA route is 261 rows, five workgroups with a ragged tile: without large counts G is a sum
# of B terms of either sign against a bound that grows with B, and at 1029 rows EPS * bound is 1.1e-3 to 1.4e-3 of the
# largest |G| at every seed tried; at 261 rows it is half of that.)
SEED_BASE = 0       # the seeds at which EPS * bound stays below 1e-3 of the results (tests/test_glm_zip_cpu.py asserts it)


def case_seed(B, D, S):
    return SEED_BASE + B * 7 + D + S


# ---- the pass -------------------------------------------------------------------------------------------------------

def logit_size(X, W, offset):
    """a[n,s] = sum_d |x_nd w_sd| + |o_n|: the size of the logit's float32 terms."""
    a = np.abs(_f64(X)) @ np.abs(_f64(W)).T
    return a if offset is None else a + np.abs(_f64(offset))[:, None]


def link(L, y64, tau):
    """(log p without the row constant, d / d l, d / d tau) per (row, draw) in float64; y64 [B, 1], tau [1, S]."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        mu = np.exp(L)
        u = tau + mu
        L1 = np.logaddexp(0.0, tau)
        zero = y64 == 0.0
        lp = np.where(zero, np.logaddexp(tau, -mu), y64 * L - mu) - L1
        dl = np.where(zero, -mu * expit(-u), y64 - mu)
        dt = np.where(zero, expit(u) * expit(-tau) * -np.expm1(-mu), -expit(tau) + 0.0 * L)
    return lp, dl, dt


def _terms(X, y, W, logodds, offset, weights):
    """Per (row, draw): the terms of ell, the residual, the terms of T, and the three bound quantities."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    y64 = _f64(y)[:, None]
    tau = _f64(logodds)[None, :]
    v = np.ones(L.shape[0]) if weights is None else _f64(weights)
    on = (v > 0.0)[:, None]
    vv = v[:, None]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        lp, dl, dt = link(L, y64, tau)
        mu = np.exp(L)
        zero = y64 == 0.0
        rr = np.where(zero, expit(-(tau + mu)), 1.0)
        t_ell = np.where(on, vv * lp, 0.0)
        a_ell = np.where(on, vv * (np.abs(tau) + mu + np.logaddexp(0.0, tau) + np.abs(y64 * L) + 1.0), 0.0)
        r = np.where(on, vv * dl, 0.0)
        a_r = np.where(on, vv * (np.abs(y64) + (1.0 + a) * mu * rr + np.where(zero, a * mu * mu * rr * (1.0 - rr), 0.0)),
                       0.0)
        t_T = np.where(on, vv * dt, 0.0)
        a_T = np.where(on, vv * (np.abs(dt) + expit(tau) + 1.0), 0.0)
    return t_ell, a_ell, r, a_r, t_T, a_T


def data_pass(X, y, W, logodds, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, _, t_T, _ = _terms(X, y, W, logodds, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, W, logodds, offset=None, weights=None):
    """(b_ell [S], b_G [S, D], b_T [S]): what the errors are measured against (module docstring), rows of weight 0 left
    out; b_G[s,d] = sum_n a_r[n,s] |x_nd|."""
    _, a_ell, _, a_r, _, a_T = _terms(X, y, W, logodds, offset, weights)
    return a_ell.sum(axis=0), a_r.T @ np.abs(_f64(X)), a_T.sum(axis=0)


def row_logpmf(L, y, logodds):
    """log p(y_n | l_ns, tau_s), the constant -lnGamma(y + 1) included: [B, S]."""
    y64 = _f64(y)[:, None]
    return link(L, y64, _f64(logodds)[None, :])[0] - gammaln(y64 + 1.0)


# ---- the device's forms in plain float32 ----------------------------------------------------------------------------------

def _fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, the sum is rounded there and once more to float32."""
    return (_f64(a) * _f64(b) + _f64(c)).astype(np.float32)


def expm1_f32(x):
    """csrc/bsc_special_f32.h's bsc_expm1_f32 in plain float32: u - 1 where |x| > 1/2, Kahan's (u - 1) x / log u below,
    x where u == 1; the hardware reciprocal as 1 / x rounded to float32."""
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
        u = np.exp(x)
        far, one = np.abs(x) > f(0.5), u == f(1.0)
        lu = np.log(np.where(one, f(2.0), u))
        q = np.where(far, f(1.0), x) * (f(1.0) / np.where(far, f(1.0), lu))
        out = _fma(u - f(1.0), q, np.where(one, x, f(0.0)))
    assert out.dtype == f
    return out


def link_f32(l, y, v, tau, real=None):
    """csrc/bsc_families.h's ZeroInflPoisson::glm_link step by step in float32 on arrays [B, S] (l), [B, 1] (y, v) and
    [1, S] (tau): returns the three terms (v log p, v d / d l, v d / d tau), each float32."""
    f = np.float32
    one, nil = f(1.0), f(0.0)
    t64 = _f64(tau)
    L1 = np.logaddexp(0.0, t64).astype(f)              # made in float64 once per launch, then rounded
    pi = expit(t64).astype(f)
    keep = v > 0 if real is None else (v > 0) & real
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        vq = np.where(keep, v, nil)
        yq = np.where(keep, y, nil)
        lq = np.where(keep, l, nil)
        mu = np.exp(lq)
        u = tau + mu
        e = np.exp(-np.abs(u))
        t = one + e
        rc = one / t
        er = e * rc
        posu = u >= 0
        su, sn = np.where(posu, rc, er), np.where(posu, er, rc)
        tiny = t == one
        lp = np.log(t) * (e / np.where(tiny, one, t - one)) + np.where(tiny, e, nil)
        em = -expm1_f32(-mu)
        z0 = np.where(yq == 0, one, nil)
        zp = one - z0
        lp0 = np.maximum(tau, -mu) + lp
        lpp = _fma(yq, lq, -mu)
        res = _fma(-mu, _fma(z0, sn, zp), yq)
        dt0 = su * (one - pi) * em
        t_ell = vq * (_fma(z0, lp0, zp * lpp) - L1)
        t_T = vq * _fma(z0, dt0, -zp * pi)
        r = vq * res
    assert t_ell.dtype == f and t_T.dtype == f and r.dtype == f
    return t_ell, r, t_T


F32_BLOCK = 64      # rows of one float32 partial: a workgroup's four 16-row tiles


def data_pass_f32(X, y, W, logodds, offset=None, weights=None):
    """The link replayed in float32 (link_f32), the logits by one float32 matrix product, float32 partials of F32_BLOCK
    rows finished in float64 (tests/_glm_weibull_ref.data_pass_f32)."""
    f = np.float32
    X, y, W, tau = (np.asarray(a, f) for a in (X, y, W, logodds))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    with np.errstate(over="ignore", invalid="ignore"):
        l = X @ W.T + o[:, None]
    assert l.dtype == f
    t_ell, r, t_T = link_f32(l, y[:, None], v[:, None], tau[None, :])
    ell, G, T = np.zeros(S), np.zeros((S, D)), np.zeros(S)
    for b in range(0, B, F32_BLOCK):
        ell += np.cumsum(t_ell[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        T += np.cumsum(t_T[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        G += np.cumsum(r[b:b + F32_BLOCK, :, None] * X[b:b + F32_BLOCK, None, :], axis=0, dtype=f)[-1]
    return ell, G, T


# ---- draws and the finish: the negative binomial's (the scalar's prior has the same form) ---------------------------------

init_lam = nb.init_lam              # m = 0 (tau = 0, pi = 1/2), rho = log 0.1
noise = nb.noise                    # bsc_blr_noise(D): [S, D + 1]
draw = nb.draw                      # (W [S, D] float32, logodds [S] float32)
log_prior_tau = nb.log_prior_tau
elbo_and_grad = nb.elbo_and_grad    # (lam, eps, W, logodds, ell, G, T, scale, prec, a0, b0)
update = nb.finish                  # bsc_glm_zip_update from given statistics: (lam', m1', m2', elbo, grad)


def step(lam, m1, m2, t, X, y, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as ZIPoissonReparamSVI does it."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, lo = draw(lam, eps)
    ell, G, T = data_pass(X, y, W, lo, offset, weights)
    return update(lam, m1, m2, t, eps, W, lo, ell, G, T, n_total / B, prec, a0, b0, lr)


def fit(X, y, S, seed, steps, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """The reference driver: ``steps`` full-batch updates from the default start.  Returns lam."""
    lam = init_lam(X.shape[1])
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, steps + 1):
        lam, m1, m2, _, _ = step(lam, m1, m2, t, X, y, S, seed, float(X.shape[0]), lr, prec, a0, b0, offset, weights)
    return lam


def simulate(B, D, seed, pi=0.3, intercept=math.log(2.0)):
    """ZIP data with an intercept column (X[:, 0] = 1, weight ``intercept``: mu = e^intercept at x = 0) and a
    structural-zero share pi.  Returns (X float32 [B, D], y float32 [B])."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    X[:, 0] = 1.0
    w = np.concatenate([[intercept], 0.5 * np.array([-0.6, 0.4, 0.3, -0.2, 0.5, -0.4, 0.1, 0.7, -0.3][:D - 1])])
    y = rs.poisson(np.exp(_f64(X) @ w)).astype(np.float32)
    y[rs.uniform(size=B) < pi] = 0.0
    return X, y


# The end-to-end fit of tests/test_glm_zip_gpu.py: simulate(4000, 8, 5), the first 3000 rows fitted, the rest held out.
E2E = dict(B=4000, fit_rows=3000, D=8, seed=5, S=8, vi_seed=31, steps=300, lr=0.02, prec=1.0, a0=1.0, b0=1.0)
# What ``fit`` (float64, on the CPU) ends at on those rows: the posterior means and standard deviations of the intercept and
# of tau, and zero_share_mean (truth: log 2 = 0.693 and 0.3; 39.4 % of the rows are zero).  tests/test_glm_zip_cpu.py
# runs the fit and holds these figures to it.
E2E_REF = dict(intercept=0.64321, intercept_sd=0.02644, tau=-0.94117, tau_sd=0.05638, zero_share=0.28080)


def zero_share_mean(mean, var, n=200001):
    """E[sigmoid(tau)], tau ~ N(mean, var), by the trapezoidal rule over +-12 standard deviations."""
    sd = math.sqrt(var)
    t = np.linspace(-12.0, 12.0, n)
    f = expit(mean + sd * t) * np.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    return float(((f[1:] + f[:-1]) * 0.5).sum() * (t[1] - t[0]))


# ---- predictive -----------------------------------------------------------------------------------------------------

def posterior_draws(lam, D, S, seed):
    """svi/predict.py's draws: Philox stream 2, step 0, [S, D + 1].  Returns (W float32 [S, D], logodds float32 [S])."""
    eps = philox.normal_draws(seed, S, D + 1, stream=2, step=0)
    return draw(lam, eps)


def _lse_mean(lp):
    m = lp.max(axis=1, keepdims=True)
    return m[:, 0] + np.log(np.exp(lp - m).sum(axis=1)) - math.log(lp.shape[1])


def predict(X, W, logodds, y=None, offset=None, weights=None):
    """mean, var (law of total variance, centred) and, with y, lpd and lpd_sum (weighted with weights)."""
    L = obs.logits(X, W, offset)
    pi = expit(_f64(logodds))[None, :]
    mu = (1.0 - pi) * np.exp(L)
    v = mu * (1.0 + pi * np.exp(L))
    mean = mu.mean(axis=1)
    out = dict(mean=mean, var=v.mean(axis=1) + ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        out["lpd"] = _lse_mean(row_logpmf(L, y, logodds))
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def zero_probability(X, W, logodds, offset=None):
    """P(y = 0 | x_n) = mean_s [ pi_s + (1 - pi_s) e^{-mu_ns} ]: [B]."""
    L = obs.logits(X, W, offset)
    pi = expit(_f64(logodds))[None, :]
    return (pi + (1.0 - pi) * np.exp(-np.exp(L))).mean(axis=1)


def predict_bounds(X, W, logodds, y=None, offset=None, weights=None):
    """tests/_glm_nb_ref.predict_bounds' construction for this family.  With a = logit_size and EPS = 2e-5:
    m = (1 - pi) mu, dm / dl = m: e_m = EPS (m a + m), the second term covering the float32 pi;  v = m (1 + pi mu),
    dv / dl = m (1 + 2 pi mu): e_v = EPS (m (1 + 2 pi mu) a + v);  log p: EPS times the pass's per-row ell quantity plus
    the row constant, |tau| + mu + L1 + |y l| + lnGamma(y + 1) + 1, maximum over the draws."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    tau = _f64(logodds)[None, :]
    pi = expit(tau)
    el = np.exp(L)
    mu = (1.0 - pi) * el
    v = mu * (1.0 + pi * el)
    e_mu = EPS * (mu * a + mu)
    e_v = EPS * (mu * (1.0 + 2.0 * pi * el) * a + v)
    mean = mu.mean(axis=1)
    dev = np.abs(mu - mean[:, None])
    out = dict(mean=e_mu.mean(axis=1),
               var=e_v.mean(axis=1) + (2.0 * dev * (e_mu + e_mu.mean(axis=1)[:, None])).mean(axis=1)
               + EPS * ((mu - mean[:, None]) ** 2).mean(axis=1))
    if y is not None:
        y64 = _f64(y)[:, None]
        e = EPS * (np.abs(tau) + el + np.logaddexp(0.0, tau) + np.abs(y64 * L) + gammaln(y64 + 1.0) + 1.0)
        out["lpd"] = e.max(axis=1)
        w = np.ones(L.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
