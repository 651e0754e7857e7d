"""Float64 numpy restatement of the Weibull route with interval and left censoring (include/bayesic_hip.h:
bsc_glm_weibull_data_pass_interval, bsc_weibull_predict_pass_interval; svi/glm_weibull.py's ``upper=``), next to
tests/_glm_weibull_ref.py, from which the logits' sizes, the draws, the finish and the moments come by import.

Device encoding: y signed as there, and upper [B]:  0 -- the row is what y says;  > 0 (y < 0) -- interval-censored on
(a, b] = (-y, upper];  < 0 -- left-censored at b = -upper (y not read).  With k = e^tau, l the log scale,
    z = k (log a - l),  E = e^z,  d = log b - log a,  Delta = E expm1(k d),  E_b = E + Delta          (interval)
    z = k (log b - l),  E = e^z,  Delta = E,  and E_a = 0 below                                        (left-censored)
    log P    = -E_a + log(-expm1(-Delta))                                   = log(S(a) - S(b))
    d / dl   = k (E_a - delta),        delta = Delta / expm1(Delta) in (0, 1)
    d / dtau = -z E_a + (z Delta + k d E_b) / expm1(Delta)
and the rows without an upper end as in tests/_glm_weibull_ref.py.  Nothing is selected here for a far upper end: in
float64 the terms behind it are below 1e-44 where the device drops them (Delta >= 103), and from Delta = 200 on they are
set to 0 so that no infinity meets a zero.

The bound quantities follow tests/_glm_weibull_ref.py's rule -- the sum of the magnitudes of the terms, with the
conditioning of every rounded intermediate on its inputs, in units of the float32 epsilon.  With a = logit_size and
c = |z| + k (|log t| + a) the absolute error of z (t the end that z is formed from), as there:
    k d:     c_d = 4 k d where b < 2 a (d comes from log1p((b - a) / a): b - a is exact, then a quotient, a log1p and
             the product with k), else k d + k (|log a| + |log b|) (two rounded logarithms)
    Delta:   relative c_D = 1 + c + g c_d,  g = e^{k d} / expm1(k d) = d log expm1(x) / dx at x = k d   (left: 1 + c)
    log p = log(-expm1(-Delta)):  d / d log Delta = delta, so it carries delta c_D and its own |log p| + 1
    delta:   Delta d delta / d Delta = delta (1 - Delta - delta) =: s
    q = 1 / expm1(Delta):  Delta dq / d Delta = -q (Delta + delta)
Per kept (row, draw), an interval or left-censored row:
    ell:  (1 + c) E_a + |log p| + delta c_D + 1
    r:    k ( (1 + c) E_a + delta + |s| c_D )
    T:    (|z| + (1 + |z|) c) E_a + |z| delta + k d E_b q + c delta + |z| |s| c_D + c_d E_b q
          + k d q (c E_a + c_D Delta) + k d E_b q (Delta + delta) c_D + 1
and a row without an upper end tests/_glm_weibull_ref.py's three.  A device result is held to EPS = 2e-5 times these, a
plain float32 evaluation (``data_pass_f32``) to F32_REACH = 1e-6 times these."""
import math

import numpy as np

import _glm_obs_ref as obs
import _glm_weibull_ref as wref

EPS = wref.EPS
TAU_LO, TAU_HI = wref.TAU_LO, wref.TAU_HI
F32_REACH = 1e-6
FAR = 1.0e30           # "no bound", written as a number
BIG = 103.0            # csrc/bsc_glm_pass.h: ITV_BIG
_f64 = obs._f64
logit_size = wref.logit_size
KINDS = ("mixed", "event", "right", "interval", "left")
# z of a row's reference time, for every draw.  A batch of events alone stops at 1: at tau = 4 an event adds
# tau + z - log t - e^z, and over (-6, 3) the mean of z - e^z is -3.7 -- the rows' terms cancel to 0.3 apiece while the
# bound quantity counts 70 apiece, so EPS times the bound is 2e-3 of ell; over (-6, 1) the mean is -2.9 and it is 6e-4.
ZETA, ZETA_EVENTS = (-6.0, 3.0), (-6.0, 1.0)

# The batches of tests/test_glm_weibull_interval_gpu.py's parity test, (B, D, S, mode, kinds), seeded B * 7 + D + S:
# tests/test_glm_weibull_interval_cpu.py holds a plain float32 evaluation, and the bounds' share of the results, at each.
PASS_BATCHES = [(1003, 12, 8, "both", "mixed"), (517, 200, 11, "both", "mixed"), (1003, 256, 3, "both", "mixed"),
                (1029, 256, 8, "both", "mixed"), (1029, 256, 11, "both", "mixed"),
                (1003, 12, 8, "both", "event"), (1003, 12, 8, "both", "right"), (1029, 256, 8, "both", "interval"),
                (1003, 12, 8, "both", "left"), (1029, 256, 8, "weights", "mixed"), (1003, 12, 8, "weights", "mixed"),
                (1029, 256, 8, "offset", "mixed"), (517, 200, 11, "offset", "mixed")]


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------

def make_inputs(B, D, S, seed, mode="both", kinds="mixed", tau=None, spread=0.01, far_every=9, w_sd=0.015, o_sd=0.1,
                zeta=None):
    """X ~ N / sqrt(D) with a first column of one sign (so that G[:, 0] is a sum that does not cancel), weights U(0, 3)
    with every fifth exactly zero, tau spread over the accuracy envelope [-2, 4] (``tau``: given), and SMALL logits:
    draws W_s = W_0 + spread N around one W_0 ~ w_sd N, as the draws of a fitted q lie around its mean, and offsets
    o_sd N.  At k = 55 the float32 logit, of size a = sum |x_d w_d| + |o|, is multiplied by 55 on its way into z, so the
    bound quantities carry 55 (|log t| + a) of every e^z: with tests/_glm_weibull_ref.py's logits (a about 7 at
    D = 256) EPS times the bounds is 1e-2 of the results themselves, with these (a below 0.5) it is below 1e-3
    (tests/test_glm_weibull_interval_cpu.py asserts it), so a device error of the bounds' size would show in the results.
    Every row's reference time is t = exp(l_0 + zeta / k_max) with zeta ~ U(``zeta``) (None: ZETA, for a batch of events
    alone ZETA_EVENTS), l_0 the first draw's logit and
    k_max the largest shape, so that z of that time lies in that range (plus the draws' spread) for EVERY draw.  Kinds, ``mixed``:
    about 40 % events at t, 20 % right-censored at t, 25 % interval-censored with the lower end t and a width
    k_max d log-uniform over [1e-4, 20] (every ``far_every``-th of them with upper = 1e30 instead), 15 % left-censored
    at t; or every row of one kind.  With weights, the rows of weight 0 hold 0, NaN and infinity in turn in y and upper.
    Returns (X, y, upper, W, logshape, offset or None, weights or None), y and upper in the device encoding."""
    assert kinds in KINDS
    if zeta is None:
        zeta = ZETA_EVENTS if kinds == "event" else ZETA
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    X[:, 0] = np.abs(X[:, 0])                              # one column of one sign: G[:, 0] is a sum that does not cancel
    W0 = w_sd * rs.standard_normal(D)
    W = (W0[None, :] + spread * rs.standard_normal((S, D))).astype(np.float32)
    o = (o_sd * rs.standard_normal(B)).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    use_o, use_v = mode in ("offset", "both"), mode in ("weights", "both")
    if tau is None:
        logshape = np.linspace(TAU_LO, TAU_HI, S)[rs.permutation(S)] if S > 1 else np.array([0.5])
    else:
        logshape = np.broadcast_to(np.asarray(tau, np.float64), (S,))
    logshape = logshape.astype(np.float32)
    k_max = float(np.exp(_f64(logshape)).max())
    L0 = obs.logits(X, W, o if use_o else None)[:, 0]
    t = np.exp(L0 + rs.uniform(zeta[0], zeta[1], B) / k_max).astype(np.float32)
    pick = rs.uniform(size=B)
    width = np.exp(rs.uniform(math.log(1e-4), math.log(20.0), B)) / k_max
    if kinds == "mixed":
        kind = np.where(pick < 0.4, 0, np.where(pick < 0.6, 1, np.where(pick < 0.85, 2, 3)))
    else:
        kind = np.full(B, KINDS.index(kinds) - 1)
    y = np.where(kind == 0, t, -t).astype(np.float32)
    upper = np.zeros(B, np.float32)
    itv = np.flatnonzero(kind == 2)
    with np.errstate(over="ignore"):                      # a width past float32 is an upper end at infinity
        b = (t[itv].astype(np.float64) * np.exp(width[itv])).astype(np.float32)
    b = np.maximum(b, np.nextafter(t[itv], np.float32(np.inf)))          # b > a as float32
    b[::far_every] = FAR
    upper[itv] = b
    left = kind == 3
    upper[left] = -t[left]
    y[left] = -t[left]
    if use_v:
        dead = np.flatnonzero(v == 0)
        for i, (hy, hu) in enumerate(((0.0, 0.0), (np.nan, np.nan), (np.inf, -np.inf), (-1.0, np.nan), (0.0, np.inf))):
            y[dead[i::5]] = hy
            upper[dead[i::5]] = hu
    return X, y, upper, W, logshape, (o if use_o else None), (v if use_v else None)


def plain_inputs(B, D, S, seed):
    """Events and right-censored rows alone (every third row an event), for the comparison of BITS with the pass without
    ``upper``; no tolerance is taken from this batch.  (X, y, W, logshape, offset, weights)."""
    X, y, _, W, logshape, o, v = make_inputs(B, D, S, seed=seed, kinds="right")
    y = np.where(np.arange(B) % 3 == 0, -y, y).astype(np.float32)
    y[~np.isfinite(y)] = 0.0                               # (rows of weight 0)
    return X, y, W, logshape, o, v


# ---- the pass -----------------------------------------------------------------------------------------------------------

def _terms(X, y, upper, W, logshape, offset, weights):
    """Per (row, draw): the terms of ell, the residual, the terms of T, and the three bound quantities (module
    docstring); rows of weight 0 give exact zeros whatever they hold."""
    L = obs.logits(X, W, offset)
    a = logit_size(X, W, offset)
    B = L.shape[0]
    v = np.ones(B) if weights is None else _f64(weights)
    on = v > 0.0
    y64 = np.where(on, _f64(y), 1.0)                      # a dropped row: an event at 1, never used
    u64 = np.where(on, _f64(upper), 0.0)
    tau = _f64(logshape)[None, :]
    k = np.exp(tau)
    vv = np.where(on, v, 0.0)[:, None]
    left, itv = (u64 < 0)[:, None], (u64 > 0)[:, None]
    cen = left | itv
    dl = ((u64 == 0) & (y64 > 0)).astype(np.float64)[:, None]
    t_lo = np.where(u64 < 0, -u64, np.abs(y64))[:, None]  # the end that z is formed from
    t_hi = np.where(u64 > 0, u64, t_lo[:, 0])[:, None]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ly, lb = np.log(t_lo), np.log(t_hi)
        z = k * (ly - L)
        ez = np.exp(z)
        az = np.abs(z)
        c = az + k * (np.abs(ly) + a)
        near = t_hi < 2.0 * t_lo                          # log1p: a narrow interval keeps its digits here as well
        kd = k * np.where(near, np.log1p((t_hi - t_lo) / t_lo), lb - ly)   # exactly 0 unless the row is an interval
        c_d = np.where(near, 4.0 * kd, kd + k * (np.abs(ly) + np.abs(lb)))
        delta_big = np.where(left, ez, ez * np.expm1(kd))
        live = cen & (delta_big < 200.0)                  # behind it every term of the upper end is below 1e-80
        Dq = np.where(live, delta_big, 1.0)
        kq = np.where(live, kd, 0.0)
        cq = np.where(live, c_d, 0.0)
        g = np.where(live & itv, 1.0 / -np.expm1(-np.where(kq > 0, kq, 1.0)), 0.0)
        c_D = 1.0 + c + g * cq
        ea = np.where(left, 0.0, ez)
        p = -np.expm1(-Dq)
        q = np.exp(-Dq) / p
        dlt = Dq * q
        s = np.abs(dlt * (1.0 - Dq - dlt))
        eb = ea + Dq
        lp = np.log(p)
        ic = live.astype(np.float64)
        t_ell = vv * (dl * (tau + z - ly) - ea + ic * lp)
        r = vv * k * (ea - dl - ic * dlt)
        t_T = vv * (dl * (1.0 + z) - z * ea + ic * (z * Dq + kq * eb) * q)
        a_ell = vv * (dl * (np.abs(tau) + az + np.abs(ly) + c) + (1.0 + c) * ea + 1.0 + ic * (np.abs(lp) + dlt * c_D))
        a_r = vv * k * ((1.0 + c) * ea + dl + ic * (dlt + s * c_D))
        a_T = vv * (dl * (1.0 + az + c) + (az + (1.0 + az) * c) * ea + 1.0
                    + ic * (az * dlt + kq * eb * q + c * dlt + az * s * c_D + cq * eb * q
                            + kq * q * (c * ea + c_D * Dq) + kq * eb * q * (Dq + dlt) * c_D))
    return t_ell, a_ell, r, a_r, t_T, a_T


def data_pass(X, y, upper, W, logshape, offset=None, weights=None):
    """(ell [S], G [S, D], T [S]): float32 operands, float64 arithmetic."""
    t_ell, _, r, _, t_T, _ = _terms(X, y, upper, W, logshape, offset, weights)
    return t_ell.sum(axis=0), r.T @ _f64(X), t_T.sum(axis=0)


def bounds(X, y, upper, W, logshape, offset=None, weights=None):
    """(b_ell [S], b_G [S, D], b_T [S]): what the errors are measured against (module docstring)."""
    _, a_ell, _, a_r, _, a_T = _terms(X, y, upper, W, logshape, offset, weights)
    return a_ell.sum(axis=0), a_r.T @ np.abs(_f64(X)), a_T.sum(axis=0)


def row_logp(X, y, upper, W, logshape, offset=None):
    """log f(a) of an event, log S(a) of a right-censored row, log(S(a) - S(b)) of an interval, log F(b) of a
    left-censored row, per (row, draw): [B, S]."""
    return _terms(X, y, upper, W, logshape, offset, None)[0]


F32_BLOCK = wref.F32_BLOCK


def _log_ratio_f32(b, a, la):
    """csrc/bsc_special_f32.h's bsc_logratio_f32, plainly: log1p((b - a) / a) where b < 2 a, else log b - log a."""
    f = np.float32
    near = b < f(2.0) * a
    r = np.where(near, b - a, f(0.0)) / a
    return np.where(near, np.log1p(r), np.log(np.where(near, f(1.0), b)) - la).astype(f)


def _link_f32(l, y, upper, tau, v):
    """The link of csrc/bsc_glm_pass.h (GLM_WEIBULL with the upper end) in plain float32, every row at once: the terms
    of ell, the residuals and the terms of T, [B, S] float32.  The selects sit where the link's sit."""
    f = np.float32
    one, zero = f(1.0), f(0.0)
    k = np.exp(tau)[None, :]
    keep = v > 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):   # every array below is float32
        vq = np.where(keep, v, zero)[:, None]
        left = keep & (upper < 0)
        itv = keep & (upper > 0)
        tq = np.where(keep, np.abs(np.where(upper < 0, upper, y)), one)
        bq = np.where(itv, upper, tq)
        dl = np.where(keep & (upper == 0) & (y > 0), one, zero)[:, None]
        ly = np.log(tq)
        d = _log_ratio_f32(bq, tq, ly)[:, None]
        ly = ly[:, None]
        z = k * (ly - np.where(keep[:, None], l, zero))
        ez = np.exp(z)
        kd = k * d
        dlt = ez * (np.expm1(kd) + np.where(left, one, zero)[:, None])
        on = (left | itv)[:, None] & (dlt < f(BIG))
        ic = np.where(on, one, zero)
        dq = np.where(on, dlt, one)
        kq = np.where(on, kd, zero)
        ea = np.where(left[:, None], zero, ez)
        p = -np.expm1(-dq)
        q = np.exp(-dq) / p
        eb = ea + dq
        t_ell = vq * (dl * ((tau[None, :] + z) - ly) + (ic * np.log(p) - ea))
        t_T = vq * (dl * (one + z) + ((ic * q) * (z * dq + kq * eb) - z * ea))
        r = vq * (k * (ea - ((ic * q) * dq + dl)))
    assert t_ell.dtype == f and t_T.dtype == f and r.dtype == f
    return t_ell, r, t_T


def data_pass_f32(X, y, upper, W, logshape, offset=None, weights=None):
    """The same formulas evaluated plainly in float32, the logits by one float32 matrix product; the sums follow the
    pass's design as tests/_glm_weibull_ref.data_pass_f32's do (float32 partials of F32_BLOCK rows, finished in
    float64)."""
    f = np.float32
    X, y, upper, W, tau = (np.asarray(a, f) for a in (X, y, upper, W, logshape))
    B, D = X.shape
    S = W.shape[0]
    o = np.zeros(B, f) if offset is None else np.asarray(offset, f)
    v = np.ones(B, f) if weights is None else np.asarray(weights, f)
    l = X @ W.T + o[:, None]
    assert l.dtype == f
    t_ell, r, t_T = _link_f32(l, y, upper, tau, v)
    ell, G, T = np.zeros(S), np.zeros((S, D)), np.zeros(S)
    for b in range(0, B, F32_BLOCK):
        ell += np.cumsum(t_ell[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        T += np.cumsum(t_T[b:b + F32_BLOCK], axis=0, dtype=f)[-1]
        G += np.cumsum(r[b:b + F32_BLOCK, :, None] * X[b:b + F32_BLOCK, None, :], axis=0, dtype=f)[-1]
    return ell, G, T


# ---- draws, the finish and the driver: tests/_glm_weibull_ref.py's ---------------------------------------------------------

init_lam, noise, draw, update = wref.init_lam, wref.noise, wref.draw, wref.update
elbo_terms_size, posterior_draws = wref.elbo_terms_size, wref.posterior_draws


def step(lam, m1, m2, t, X, y, upper, S, seed, n_total, lr, prec=1.0, a0=1.0, b0=1.0, offset=None, weights=None):
    """One whole update on one mini-batch (draw of Philox step t - 1 -> pass -> finish), as WeibullReparamSVI does it
    with ``upper`` set; y and upper in the device encoding."""
    B, D = X.shape
    eps = noise(D, S, seed, t - 1)
    W, logshape = draw(lam, eps)
    ell, G, T = data_pass(X, y, upper, W, logshape, offset, weights)
    return update(lam, m1, m2, t, eps, W, logshape, ell, G, T, n_total / B, prec, a0, b0, lr)


# ---- predictive ---------------------------------------------------------------------------------------------------------

def predict(X, W, logshape, y=None, upper=None, offset=None, weights=None):
    """mean and var as tests/_glm_weibull_ref.predict (they do not depend on the row's kind) and, with y and upper, lpd
    -- the log of the draw average of the row's density or probability -- and lpd_sum (weighted with weights)."""
    out = wref.predict(X, W, logshape, None, offset)
    if y is not None:
        lp = _terms(X, y, upper, W, logshape, offset, None)[0]
        out["lpd"] = wref._lse_mean(lp)
        w = np.ones(X.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out


def predict_bounds(X, W, logshape, y=None, upper=None, offset=None, weights=None):
    """tests/_glm_weibull_ref.predict_bounds for mean and var; lpd: EPS times the pass's per-row ell quantity (module
    docstring), maximum over the draws."""
    out = wref.predict_bounds(X, W, logshape, None, offset)
    if y is not None:
        a_ell = _terms(X, y, upper, W, logshape, offset, None)[1]
        out["lpd"] = EPS * a_ell.max(axis=1)
        w = np.ones(X.shape[0]) if weights is None else _f64(weights)
        out["lpd_sum"] = (w * out["lpd"]).sum()
    return out
