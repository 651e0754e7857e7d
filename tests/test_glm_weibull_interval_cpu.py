"""The float64 reference of the Weibull route with interval and left censoring (tests/_glm_weibull_interval_ref.py) checked
against scipy and itself, what a plain float32 evaluation reaches against the device bounds, and the driver's host side;
no device needed.

 * log P of an interval row against log(sf(a) - sf(b)) of scipy.stats.weibull_min for k d >= 1e-3, of a left-censored row
   against logcdf, rtol 1e-9;
 * a narrow interval (k d = 2 log1p(2^-21), about 1e-6, with b - a exact) against logpdf(a) + log(b - a): the tolerance is
   twice the difference between the result at that width and at half the width, the truncation term.  The point is
   k = 2, a = e^l = 1, where the first two terms of log((1/h) int_a^{a+h} f) - log f(a) = c_1 h + c_2 h^2 have one sign
   (c_1 = (log f)'/2 = -1/2, c_2 = (log f)'^2/24 + (log f)''/6 = 1/24 - 1/2): the stated tolerance is c_1 h + 3/2 c_2 h^2
   against an error of c_1 h + c_2 h^2, so it can only hold where they do not pull against each other;
 * G and T against central differences of the reference's own ell, tests/test_glm_weibull_cpu.py's two-step-size
   tolerance and its non-vacuity assertion;
 * an all-zero upper is tests/_glm_weibull_ref.data_pass (rtol 1e-13); upper = 1e30 gives the right-censored values,
   finite, in data_pass_f32 too; zero-weight rows holding 0, NaN or infinity in y and upper change nothing;
 * data_pass_f32 within F32_REACH = 1e-6 of the bound quantities at every shape tests/test_glm_weibull_interval_gpu.py
   runs and at tau in {-2, 4}, and the bounds are not vacuous there: EPS x bound <= 1e-3 of |ell|, max |G|, max |T|;
 * the driver's refusals, each naming the row kind and before a device is asked for, and the packing."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.stats import weibull_min

import _glm_weibull_interval_ref as ref
import _glm_weibull_ref as wref


def _rows(l, a, b, tau, left=False):
    """One-column inputs whose logit is l (float64 throughout): an interval (a, b] or a left-censored row at b per row."""
    B = len(l)
    X = np.asarray(l, np.float64)[:, None]
    W = np.ones((1, 1))
    y = -np.asarray(b if left else a, np.float64)
    upper = -np.asarray(b, np.float64) if left else np.asarray(b, np.float64)
    return X, y, upper, W, np.full(1, tau), B


def test_log_probability_of_interval_and_left_rows_is_scipys():
    rs = np.random.RandomState(0)
    n = 2000
    tau = rs.uniform(-2.0, 4.0, n)
    z_a = rs.uniform(-6.0, 3.0, n)
    kd = np.exp(rs.uniform(math.log(1e-3), 3.0, n))
    l = rs.uniform(-2.0, 2.0, n)
    worst = 0.0
    def f32(x):                                                              # the reference takes float32 operands
        with np.errstate(over="ignore"):                                     # (a width past float32: b at infinity)
            return float(np.float32(x))

    tau, l = tau.astype(np.float32).astype(np.float64), l.astype(np.float32).astype(np.float64)
    for i in range(n):
        k = math.exp(tau[i])
        a = f32(math.exp(l[i] + z_a[i] / k))
        b = f32(a * math.exp(kd[i] / k))
        X, y, upper, W, ls, _ = _rows([l[i]], [a], [b], tau[i])
        got = ref.row_logp(X, y, upper, W, ls)[0, 0]
        want = math.log(weibull_min.sf(a, k, scale=math.exp(l[i])) - weibull_min.sf(b, k, scale=math.exp(l[i])))
        worst = max(worst, abs(got - want) / abs(want))
        npt.assert_allclose(got, want, rtol=1e-9)
        # left-censored at z_b <= 2.5: behind it scipy's own log(cdf) has lost the ninth digit (cdf = 1 - 2e-9 at z_b = 3)
        bl = f32(math.exp(l[i] + min(z_a[i], 2.5) / k))
        X, y, upper, W, ls, _ = _rows([l[i]], None, [bl], tau[i], left=True)
        got = ref.row_logp(X, y, upper, W, ls)[0, 0]
        npt.assert_allclose(got, weibull_min.logcdf(bl, k, scale=math.exp(l[i])), rtol=1e-9)
    print("interval rows: worst relative difference to scipy %.3g" % worst)


def test_a_narrow_interval_is_the_density_times_its_width():
    tau, l, a = float(np.float32(math.log(2.0))), 0.0, 1.0                  # float32 operands: k = e^tau is 2 to 3e-8

    def result(h):
        X, y, upper, W, ls, _ = _rows([l], [a], [a + h], tau)
        return ref.row_logp(X, y, upper, W, ls)[0, 0] - math.log(h)          # b - a = h exactly

    h = 2.0 ** -21
    assert abs(math.exp(tau) * math.log1p(h) - 1e-6) < 1e-7                  # k d
    at, half = result(h), result(h / 2)
    want = weibull_min.logpdf(a, math.exp(tau), scale=math.exp(l))
    tol = 2.0 * abs(at - half)
    print("narrow interval: result %.15g, density %.15g, error %.3g, tolerance %.3g" % (at, want, abs(at - want), tol))
    assert abs(at - want) <= tol
    assert 0.0 < tol < 1e-6                                                  # and the tolerance is the truncation term


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 80, 4, 3
    X, y, upper, W, logshape, o, v = ref.make_inputs(B, D, S, 1, tau=[-1.0, 0.25, 1.25], spread=0.2, w_sd=0.6, o_sd=1.0)
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)       # w +- h and tau +- h exact in float32
    W, logshape = q(W), q(logshape)
    kept = v > 0
    assert (upper[kept] > 0).any() and (upper[kept] < 0).any() and (upper[kept] == 0).any()
    _, G, T = ref.data_pass(X, y, upper, W, logshape, o, v)
    b_ell = ref.bounds(X, y, upper, W, logshape, o, v)[0]

    def quotient(s, d, h):
        Wp, Wm, tp, tm = W.copy(), W.copy(), logshape.copy(), logshape.copy()
        if d is None:
            tp[s] += h
            tm[s] -= h
        else:
            Wp[s, d] += h
            Wm[s, d] -= h
        return (ref.data_pass(X, y, upper, Wp, tp, o, v)[0][s] - ref.data_pass(X, y, upper, Wm, tm, o, v)[0][s]) / (2 * h)

    h = 2.0 ** -8
    for s in range(S):
        for d in list(range(D)) + [None]:
            coarse, fine = quotient(s, d, h), quotient(s, d, h / 2)
            tol = abs(coarse - fine) + 1e-12 * b_ell[s] / h          # truncation, and the rounding of ell over 2 h
            got = T[s] if d is None else G[s, d]
            assert abs(got - fine) <= tol, (s, d, got, fine, tol)
            assert tol <= 1e-3 * max(abs(got), 1.0)                  # the check is not vacuous
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_an_all_zero_upper_is_the_model_without_it():
    X, y, W, logshape, o, v = wref.make_inputs(120, 8, 5, 3)
    got = ref.data_pass(X, y, np.zeros(120, np.float32), W, logshape, o, v)
    want = wref.data_pass(X, y, W, logshape, o, v)
    for g, w in zip(got, want):
        npt.assert_allclose(g, w, rtol=1e-13, atol=1e-13 * np.abs(w).max())
    gb, wb = ref.bounds(X, y, np.zeros(120, np.float32), W, logshape, o, v), wref.bounds(X, y, W, logshape, o, v)
    for g, w in zip(gb, wb):
        npt.assert_allclose(g, w, rtol=1e-13)


def test_a_far_upper_end_gives_the_right_censored_values_finite():
    X, y, upper, W, logshape, o, v = ref.make_inputs(200, 8, 6, 5, kinds="interval", far_every=1)
    kept = v > 0
    assert (upper[kept] == np.float32(ref.FAR)).all() and (y[kept] < 0).all()
    want = wref.data_pass(X, y, W, logshape, o, v)                    # the same rows, right-censored at -y
    got = ref.data_pass(X, y, upper, W, logshape, o, v)
    got32 = ref.data_pass_f32(X, y, upper, W, logshape, o, v)
    want32 = wref.data_pass_f32(X, np.where(kept, y, 1.0).astype(np.float32), W, logshape, o, v)
    bnd = ref.bounds(X, y, upper, W, logshape, o, v)
    for g, w, g32, w32, b in zip(got, want, got32, want32, bnd):
        assert np.isfinite(g).all() and np.isfinite(g32).all()
        npt.assert_allclose(g, w, rtol=1e-13, atol=1e-13 * np.abs(w).max())
        assert (np.abs(g32 - w32) <= 1e-7 * b).all()                  # the same float32 terms, summed in the same order
    # a left-censored row far out adds nothing: its probability is 1
    yl, ul = y.copy(), np.where(kept, -np.float32(ref.FAR), upper).astype(np.float32)
    for g, g32 in zip(ref.data_pass(X, yl, ul, W, logshape, o, v), ref.data_pass_f32(X, yl, ul, W, logshape, o, v)):
        assert (g == 0).all() and (g32 == 0).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, upper, W, logshape, o, v = ref.make_inputs(60, 8, 4, 3)
    v[50:] = 0.0
    y[50:] = [0.0, np.nan, np.inf, -0.0, 1.0, -1.0, np.nan, 0.0, -np.inf, 2.0]
    upper[50:] = [0.0, np.nan, np.inf, np.nan, np.inf, 0.0, -np.inf, -1.0, 1.0, np.nan]
    keep = v > 0
    a = ref.data_pass(X, y, upper, W, logshape, o, v)
    b = ref.data_pass(X[keep], y[keep], upper[keep], W, logshape, o[keep], v[keep])
    a32 = ref.data_pass_f32(X, y, upper, W, logshape, o, v)
    b32 = ref.data_pass_f32(X[keep], y[keep], upper[keep], W, logshape, o[keep], v[keep])
    bnd = ref.bounds(X, y, upper, W, logshape, o, v)
    for p, q, p32, q32, bb in zip(a, b, a32, b32, bnd):
        assert np.isfinite(p).all() and np.isfinite(p32).all()
        npt.assert_allclose(p, q, rtol=1e-13, atol=1e-13 * np.abs(q).max())
        assert (np.abs(p32 - q32) <= 2.0 * ref.F32_REACH * bb).all()  # (the float32 partials group other rows)
    dead = v == 0
    assert dead.sum() >= 10 and np.isnan(upper[dead]).any() and np.isinf(upper[dead]).any() and (y[dead] == 0).any()


# ---- what float32 reaches, and that the bounds say something ------------------------------------------------------------------

MI355X_CUS = 256      # tests/test_glm_weibull_interval_gpu.py sizes two batches from the device's CU count

GPU_SHAPES = [(1003, 12, 8), (517, 200, 11), (1003, 256, 3), (1029, 256, 8), (1029, 256, 11),
              (MI355X_CUS * 4 * 16 * 2 + 5, 256, 8), (MI355X_CUS * 4 * 8 * 2 + 3, 12, 8)]


def _f32_and_vacuity(X, y, upper, W, logshape, o, v, what):
    got = ref.data_pass_f32(X, y, upper, W, logshape, o, v)
    want = ref.data_pass(X, y, upper, W, logshape, o, v)
    bnd = ref.bounds(X, y, upper, W, logshape, o, v)
    assert all(np.isfinite(g).all() for g in got) and all(np.isfinite(w).all() for w in want)
    ratios = [float((np.abs(g - w) / b).max()) for g, w, b in zip(got, want, bnd)]
    ell, G, T = want
    share = [float((ref.EPS * bnd[0] / np.abs(ell)).max()),
             float((ref.EPS * bnd[1]).max() / np.abs(G).max()),
             float((ref.EPS * bnd[2]).max() / np.abs(T).max())]
    print("%s: float32 error / bound quantity ell %.3g, G %.3g, T %.3g; EPS x bound / size ell %.3g, G %.3g, T %.3g" % (
        what, *ratios, *share))
    assert max(ratios) <= ref.F32_REACH, ratios
    assert max(share) <= 1e-3, share


@pytest.mark.parametrize("B,D,S,mode,kinds", ref.PASS_BATCHES + [s + ("both", "mixed") for s in GPU_SHAPES[-2:]])
def test_plain_float32_stays_inside_the_bounds_at_the_gpu_shapes(B, D, S, mode, kinds):
    """Every batch of the GPU parity test (the same inputs: ref.PASS_BATCHES) and its two batches sized from the CU count."""
    X, y, upper, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode, kinds=kinds)
    assert ref.TAU_LO <= logshape.min() and logshape.max() <= ref.TAU_HI
    assert (o is None) == (mode == "weights") and (v is None) == (mode == "offset")
    if kinds == "mixed":
        kept = np.ones(B, bool) if v is None else v > 0
        shares = [((upper[kept] == 0) & (y[kept] > 0)).mean(), ((upper[kept] == 0) & (y[kept] < 0)).mean(),
                  (upper[kept] > 0).mean(), (upper[kept] < 0).mean()]
        assert all(abs(s - w) < 0.06 for s, w in zip(shares, (0.4, 0.2, 0.25, 0.15))), shares
        assert (upper[kept] == np.float32(ref.FAR)).any()
    _f32_and_vacuity(X, y, upper, W, logshape, o, v, "B=%d D=%d S=%d %s %s" % (B, D, S, mode, kinds))


@pytest.mark.parametrize("tau", [ref.TAU_LO, ref.TAU_HI])
def test_plain_float32_stays_inside_the_bounds_at_the_corners_of_the_envelope(tau):
    """At tau = -2 the times are spread over e^{+-22} (zeta / k with k = 0.135); zeta is centred there, so that the events'
    -log t does not cancel the censored rows' negative terms in ell."""
    X, y, upper, W, logshape, o, v = ref.make_inputs(1003, 12, 8, seed=11, tau=tau,
                                                     zeta=(-3.0, 3.0) if tau < 0 else (-6.0, 3.0))
    assert (logshape == np.float32(tau)).all()
    _f32_and_vacuity(X, y, upper, W, logshape, o, v, "tau=%g" % tau)


# ---- the driver's host side ---------------------------------------------------------------------------------------------------

def test_packing_gives_the_device_encoding():
    import torch
    from bayesic_amd.svi.glm_weibull import pack_censored, pack_response
    inf = np.inf
    time = np.array([1.5, 2.0, 0.5, 0.0, 3.0, 4.0], np.float32)
    event = np.array([1, 0, 0, 0, 1, 0])
    upper = np.array([inf, inf, 0.75, 2.5, inf, 1e30])
    want_y = np.array([1.5, -2.0, -0.5, -2.5, 3.0, -4.0], np.float32)
    want_u = np.array([0.0, 0.0, 0.75, -2.5, 0.0, 1e30], np.float32)
    y, u = pack_censored(time, event, upper)
    assert y.dtype == np.float32 and u.dtype == np.float32
    npt.assert_array_equal(y, want_y)
    npt.assert_array_equal(u, want_u)
    # event=None: a row with a finite upper is censored, every other row is an event
    y, u = pack_censored(time, None, upper)
    npt.assert_array_equal(y, np.array([1.5, 2.0, -0.5, -2.5, 3.0, -4.0], np.float32))
    npt.assert_array_equal(u, want_u)
    # tensors give tensors
    y, u = pack_censored(torch.from_numpy(time), torch.from_numpy(event), torch.from_numpy(upper))
    assert y.dtype == torch.float32 and u.dtype == torch.float32
    npt.assert_array_equal(y.numpy(), want_y)
    npt.assert_array_equal(u.numpy(), want_u)
    # upper=None: pack_response's result, and no second vector
    y, u = pack_censored(time[:3], event[:3], None)
    npt.assert_array_equal(y, pack_response(time[:3], event[:3]))
    assert u is None


def test_refusals_name_the_row_kind_and_need_no_device():
    from bayesic_amd.svi import WeibullReparamSVI
    inf = np.inf
    X = np.zeros((5, 4), np.float32)
    time = np.array([1.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    ok = np.array([inf, 2.5, inf, inf, inf])

    def upper(i, value):
        u = ok.copy()
        u[i] = value
        return u

    for u, match in ((upper(1, 2.0), "an interval-censored row needs upper > time"),
                     (upper(1, 1.5), "an interval-censored row needs upper > time"),
                     (upper(2, np.nan), "upper must not be NaN"),
                     (upper(2, -1.0), "upper must not be negative"),
                     (ok[:4], "upper must be a float array of length 5"),
                     (np.arange(5), "upper must be a float array of length 5")):
        with pytest.raises(ValueError, match=match):
            WeibullReparamSVI(X, time, upper=u)
    with pytest.raises(ValueError, match="an event row .* cannot have a finite upper"):
        WeibullReparamSVI(X, time, event=np.array([1, 1, 1, 1, 1]), upper=ok)
    # time == 0 belongs to a left-censored row alone
    t0 = time.copy()
    t0[3] = 0.0
    with pytest.raises(ValueError, match="only a left-censored row .* may have time == 0"):
        WeibullReparamSVI(X, t0, upper=ok)
    with pytest.raises(ValueError, match="a left-censored row .* needs a finite upper > 0"):
        WeibullReparamSVI(X, t0, upper=upper(3, 0.0))
    # a float64 tensor pair that collapses to b == a in float32 is refused as such: the device reads float32
    import torch
    from bayesic_amd.svi.glm_weibull import pack_censored
    with pytest.raises(ValueError, match="an interval-censored row needs upper > time"):
        pack_censored(torch.tensor([1.0], dtype=torch.float64), None, torch.tensor([1.0 + 1e-9], dtype=torch.float64))
    y64, u64 = pack_censored(torch.tensor([1.0], dtype=torch.float64), None, torch.tensor([1.5], dtype=torch.float64))
    assert y64.dtype == torch.float32 and u64.dtype == torch.float32
    # without upper every message is the one it was
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        WeibullReparamSVI(X, t0)
    with pytest.raises(ValueError, match="upper= needs time="):
        WeibullReparamSVI.__new__(WeibullReparamSVI).predict(X, upper=ok)


def test_set_batch_keeps_the_pair_and_the_pass_follows_it():
    import torch
    from bayesic_amd.svi import WeibullReparamSVI
    m = WeibullReparamSVI.__new__(WeibullReparamSVI)
    m.D, m.ctx = 4, None
    X = torch.zeros((4, 4))
    time = torch.tensor([1.0, 2.0, 0.0, 3.0])
    up = torch.tensor([np.inf, 2.5, 4.0, np.inf])
    m.set_batch(X, time, upper=up)
    npt.assert_array_equal(m.y.numpy(), np.array([1.0, -2.0, -4.0, 3.0], np.float32))
    npt.assert_array_equal(m.upper.numpy(), np.array([0.0, 2.5, -4.0, 0.0], np.float32))
    assert m._uarg is m.upper and m.B == 4
    calls = []

    class Ctx:
        def call(self, name, *a):
            calls.append((name, a))

    m.ctx, m._W, m._logshape, m.t, m.S, m.ell, m.G, m.T = Ctx(), torch.zeros((2, 4)), torch.zeros((2, 1)), 0, 1, None, None, None
    m.data_pass()
    assert calls[-1][0] == "bsc_glm_weibull_data_pass_interval" and calls[-1][1][3] is m.upper
    m.set_batch(X, time[[0, 1, 3, 3]])                    # the next batch has none: the pass it always was
    assert m.upper is None and m._uarg is None
    m.data_pass()
    assert calls[-1][0] == "bsc_glm_weibull_data_pass" and len(calls[-1][1]) == 13
    m.set_batch(1234, 5678, rows=4, upper=91011)
    assert m._uarg == 91011 and m.upper is None
    with pytest.raises(ValueError, match="upper must not be NaN"):
        m.set_batch(X, time, upper=torch.tensor([np.inf, np.nan, 4.0, np.inf]))


def test_predict_takes_upper_for_the_weibull_family_only():
    from bayesic_amd.svi import GammaReparamSVI
    from bayesic_amd.svi import predict as mod
    g = GammaReparamSVI.__new__(GammaReparamSVI)
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not gamma"):
        mod.predict(g, np.zeros((3, 4), np.float32), np.ones(3, np.float32), upper=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not gamma"):
        mod.heldout_lpd(g, np.zeros((3, 4), np.float32), np.ones(3, np.float32), upper=np.zeros(3, np.float32))
    assert mod.SCALAR_PASSES["weibull"] == "bsc_weibull_predict_pass" and set(mod.FAMILIES) == {"gaussian", "logistic",
                                                                                                   "poisson"}
