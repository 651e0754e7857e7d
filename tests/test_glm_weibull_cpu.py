"""The float64 reference of the Weibull survival route (tests/_glm_weibull_ref.py) checked against scipy and itself, what
a float32 pass can reach against the device bounds, and the driver's host side; no device needed.

 * log f and log S against scipy.stats.weibull_min.logpdf and .logsf (c = k, scale = e^l), rtol 1e-10;
 * G and T against central differences of the reference's own ell in w and tau on a batch of events and censored rows;
   the tolerance is the difference between the quotients at h and h / 2 (three times the finer one's truncation error);
 * tau = 0 with every row an event: ell and G are tests/_glm_gamma_ref.py's at tau = 0;
 * a censored-only batch has every residual >= 0; a zero-weight row holding 0 or NaN changes nothing;
 * the predictive moments against weibull_min.mean and .var, survival against the draw average of weibull_min.sf;
 * data_pass_f32 (plain float32) within 1e-6 of the bound quantities at every shape tests/test_glm_weibull_gpu.py runs
   (its two batches sized from the CU count at 256 CUs) and at the corners of the envelope: tau in {-2, 4}, z up to 80;
 * the constructor's refusals, each before a device is asked for, and the packing where(event, time, -time)."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.stats import weibull_min

import _glm_gamma_ref as gref
import _glm_obs_ref as obs
import _glm_weibull_ref as ref

F32_REACH = 1e-6        # what a plain float32 evaluation is held to, of the bound quantities (the device: ref.EPS = 2e-5)


def test_row_logpdf_is_scipys_weibull_density_and_survival():
    X, y, W, logshape, o, _ = ref.make_inputs(200, 8, 6, 2, mode="offset")
    L = obs.logits(X, W, o)
    k = np.exp(logshape.astype(np.float64))[None, :]
    t = np.abs(y.astype(np.float64))[:, None]
    event = (y > 0)[:, None]
    want = np.where(event, weibull_min.logpdf(t, k, scale=np.exp(L)), weibull_min.logsf(t, k, scale=np.exp(L)))
    npt.assert_allclose(ref.row_logpdf(L, y, logshape), want, rtol=1e-10)
    assert 40 < (y < 0).sum() < 80 and logshape.min() == -2.0 and logshape.max() == 4.0
    # and ell is its sum: nothing is left out
    ell, _, _ = ref.data_pass(X, y, W, logshape, o, None)
    npt.assert_allclose(ell, want.sum(axis=0), rtol=1e-10)


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 60, 4, 3
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, 1, z_max=2.0, tau=[-1.0, 0.25, 1.25])
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)       # w +- h and tau +- h exact in float32
    W, logshape = q(W), q(logshape)
    assert (y[v > 0] > 0).any() and (y[v > 0] < 0).any()
    _, G, T = ref.data_pass(X, y, W, logshape, o, v)
    b_ell = ref.bounds(X, y, W, logshape, o, v)[0]

    def quotient(s, d, h):
        Wp, Wm, tp, tm = W.copy(), W.copy(), logshape.copy(), logshape.copy()
        if d is None:
            tp[s] += h
            tm[s] -= h
        else:
            Wp[s, d] += h
            Wm[s, d] -= h
        return (ref.data_pass(X, y, Wp, tp, o, v)[0][s] - ref.data_pass(X, y, Wm, tm, o, v)[0][s]) / (2 * h)

    h = 2.0 ** -8
    for s in range(S):
        for d in list(range(D)) + [None]:
            coarse, fine = quotient(s, d, h), quotient(s, d, h / 2)
            tol = abs(coarse - fine) + 1e-12 * b_ell[s] / h          # truncation, and the rounding of ell over 2 h
            got = T[s] if d is None else G[s, d]
            assert abs(got - fine) <= tol, (s, d, got, fine, tol)
            assert tol <= 1e-3 * max(abs(got), 1.0)                  # the check is not vacuous
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_at_unit_shape_with_every_row_an_event_ell_and_G_are_the_gamma_models():
    X, y, W, _, o, v = ref.make_inputs(120, 8, 4, 3, censored=0.0, tau=0.0)
    keep = v > 0
    y = np.where(keep, y, 1.0).astype(np.float32)                    # the Gamma reference takes no NaN
    assert (y > 0).all()
    tau = np.zeros(4, np.float32)
    ell, G, T = ref.data_pass(X, y, W, tau, o, v)
    ell_g, G_g, T_g = gref.data_pass(X, y, W, tau, o, v)
    npt.assert_allclose(ell, ell_g, rtol=1e-12)
    npt.assert_allclose(G, G_g, rtol=1e-12, atol=1e-12 * np.abs(G_g).max())
    assert np.abs(T - T_g).min() > 1e-3                               # T does not coincide


def test_a_censored_only_batch_pushes_every_scale_up():
    X, y, W, logshape, o, v = ref.make_inputs(90, 8, 5, 4, censored=1.0)
    assert (y[v > 0] < 0).all()
    r = ref._terms(X, y, W, logshape, o, v)[2]
    assert (r >= 0).all() and (r[v > 0] > 0).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, logshape, o, v = ref.make_inputs(40, 8, 4, 3)
    v[36:] = 0.0
    y[36:] = [0.0, np.nan, np.inf, -0.0]
    o[36:] = [200.0, -1.0e30, 1.0e30, 0.0]
    keep = v > 0
    a = ref.data_pass(X, y, W, logshape, o, v)
    b = ref.data_pass(X[keep], y[keep], W, logshape, o[keep], v[keep])
    a32 = ref.data_pass_f32(X, y, W, logshape, o, v)
    for p, q, p32 in zip(a, b, a32):
        assert np.isfinite(p).all() and np.isfinite(p32).all()
        npt.assert_allclose(p, q, rtol=1e-13, atol=1e-13 * np.abs(q).max())
    assert (v == 0).sum() >= 10 and np.isnan(y[v == 0]).any() and (y[v == 0] == 0).any()


def test_predictive_reference_against_scipy():
    B, D, S = 120, 8, 16
    X, y, W, logshape, o, _ = ref.make_inputs(B, D, S, 4, mode="offset")
    out = ref.predict(X, W, logshape, y, o)
    L = obs.logits(X, W, o)
    k = np.exp(logshape.astype(np.float64))[None, :]
    m = weibull_min.mean(k, scale=np.exp(L))
    v = weibull_min.var(k, scale=np.exp(L))
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-10)
    npt.assert_allclose(out["var"], v.mean(axis=1) + m.var(axis=1), rtol=1e-8)       # law of total variance
    t = np.abs(y.astype(np.float64))[:, None]
    lp = np.where((y > 0)[:, None], weibull_min.logpdf(t, k, scale=np.exp(L)), weibull_min.logsf(t, k, scale=np.exp(L)))
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    # survival: the draw average of scipy's sf, and exp(lpd) of the batch with every row censored
    npt.assert_allclose(ref.survival(X, W, logshape, t[:, 0], o), weibull_min.sf(t, k, scale=np.exp(L)).mean(axis=1),
                        rtol=1e-10, atol=1e-300)
    npt.assert_allclose(np.exp(ref.predict(X, W, logshape, -t[:, 0], o)["lpd"]), ref.survival(X, W, logshape, t[:, 0], o),
                        rtol=1e-10, atol=1e-300)
    b = ref.predict_bounds(X, W, logshape, y, o)
    assert all((b[q] > 0).all() for q in ("mean", "var", "lpd")) and b["lpd_sum"] > 0


# ---- what float32 reaches ---------------------------------------------------------------------------------------------

def _f32_ratios(X, y, W, logshape, o, v):
    got = ref.data_pass_f32(X, y, W, logshape, o, v)
    want = ref.data_pass(X, y, W, logshape, o, v)
    bnd = ref.bounds(X, y, W, logshape, o, v)
    assert all(np.isfinite(g).all() for g in got)
    return [float((np.abs(g - w) / b).max()) for g, w, b in zip(got, want, bnd)]


MI355X_CUS = 256      # tests/test_glm_weibull_gpu.py sizes two batches from the device's CU count

GPU_SHAPES = [(1003, 12, 8), (517, 200, 11), (1003, 256, 3), (1029, 256, 8), (1029, 256, 11),
              (MI355X_CUS * 4 * 16 * 2 + 5, 256, 8), (MI355X_CUS * 4 * 8 * 2 + 3, 12, 8)]


@pytest.mark.parametrize("B,D,S,censored", [s + (0.3,) for s in GPU_SHAPES] + [(1003, 12, 8, 0.0), (1003, 12, 8, 1.0)])
def test_plain_float32_stays_inside_the_bounds_at_the_gpu_shapes(B, D, S, censored):
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, censored=censored)
    r_ell, r_G, r_T = _f32_ratios(X, y, W, logshape, o, v)
    print("B=%d D=%d S=%d censored %.1f: error / bound quantity ell %.3g, G %.3g, T %.3g" % (
        B, D, S, censored, r_ell, r_G, r_T))
    assert max(r_ell, r_G, r_T) <= F32_REACH
    assert ref.TAU_LO <= logshape.min() and logshape.max() <= ref.TAU_HI


@pytest.mark.parametrize("tau", [ref.TAU_LO, ref.TAU_HI])
def test_plain_float32_stays_inside_the_bounds_at_the_corners_of_the_envelope(tau):
    """z from -80 to just below 80 at log t in {-80, -5, 0, 5, 80}; the logit is l = log t - z / k, almost all of it
    through the offset: |l| reaches 80 + 80 / k, about 670 at tau = -2 (the pass never forms e^l)."""
    rs = np.random.RandomState(7)
    B, D, S = 640, 8, 2
    k = math.exp(tau)
    z = np.tile(np.linspace(-80.0, 78.5, B // 5), 5)
    ly = np.repeat([-80.0, -5.0, 0.0, 5.0, 80.0], B // 5)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.01 / max(k, 1.0) * rs.standard_normal((S, D))).astype(np.float32)
    o = (ly - z / k).astype(np.float32)
    y = np.exp(ly).astype(np.float32)
    y[rs.uniform(size=B) < 0.3] *= -1.0
    v = rs.uniform(0.5, 2.0, B).astype(np.float32)
    logshape = np.full(S, tau, np.float32)
    z_real = k * (np.log(np.abs(y.astype(np.float64)))[:, None] - obs.logits(X, W, o))
    assert 78.0 < z_real.max() < 80.0 and z_real.min() < -79.0 and np.abs(o).max() > 80.0 + 79.0 / k
    r_ell, r_G, r_T = _f32_ratios(X, y, W, logshape, o, v)
    print("tau=%g: error / bound quantity ell %.3g, G %.3g, T %.3g" % (tau, r_ell, r_G, r_T))
    assert max(r_ell, r_G, r_T) <= F32_REACH


# ---- the driver's host side ---------------------------------------------------------------------------------------------

def test_constructor_refusals_need_no_device():
    from bayesic_amd.svi import WeibullReparamSVI
    X = np.zeros((5, 4), np.float32)
    time = np.arange(1, 6, dtype=np.float32)
    for wrong in (0.0, -1.0, np.nan, np.inf):
        bad = time.copy()
        bad[2] = wrong
        with pytest.raises(ValueError, match="time must be finite and > 0"):
            WeibullReparamSVI(X, bad)
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        WeibullReparamSVI(X, time, np.ones(4, bool))
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        WeibullReparamSVI(X, time, event=np.array([0, 1, 2, 0, 1]))
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        WeibullReparamSVI(X, time, event=np.array([0.0, 1.0, 0.5, 0.0, 1.0]))
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        WeibullReparamSVI(X, time, lam0=np.zeros(8))
    with pytest.raises(ValueError, match="a0 and b0"):
        WeibullReparamSVI(X, time, a0=0.0)
    with pytest.raises(ValueError, match="a0 and b0"):
        WeibullReparamSVI(X, time, b0=-1.0)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        WeibullReparamSVI(X, time, prior_precision=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        WeibullReparamSVI(X, time, n_samples=65)
    with pytest.raises(TypeError):
        WeibullReparamSVI(X, time, exposure=np.ones(5, np.float32))         # there is no exposure keyword


def test_the_packing_is_where_event_time_minus_time():
    import torch
    from bayesic_amd.svi.glm_weibull import WeibullReparamSVI, pack_response
    time = np.array([0.5, 2.0, 3.0, 4.0, 1.0e-3], np.float32)
    event = np.array([1, 0, 1, 0, 0])
    want = np.array([0.5, -2.0, 3.0, -4.0, -1.0e-3], np.float32)
    for ev in (event, event.astype(bool), event.astype(np.float32), list(event), torch.from_numpy(event)):
        got = pack_response(time, ev)
        assert got.dtype == np.float32
        npt.assert_array_equal(got, want)
    npt.assert_array_equal(pack_response(time), time)                        # None: every row an event
    got = pack_response(torch.from_numpy(time), torch.from_numpy(event.astype(bool)))
    assert got.dtype == torch.float32
    npt.assert_array_equal(got.numpy(), want)
    # set_batch: the signed vector is what reaches the driver (a model that was never given a device)
    m = WeibullReparamSVI.__new__(WeibullReparamSVI)
    m.D, m.ctx = 4, None
    X = torch.zeros((5, 4))
    m.set_batch(X, torch.from_numpy(time), event=event)
    npt.assert_array_equal(m.y.numpy(), want)
    assert m._yarg is m.y and m.B == 5 and m.offset is None and m.weights is None
    for wrong in (0.0, -2.0, float("nan"), float("inf")):
        bad = torch.from_numpy(time.copy())
        bad[3] = wrong
        with pytest.raises(ValueError, match="time must be finite and > 0"):
            m.set_batch(X, bad)
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        m.set_batch(X, torch.from_numpy(time), event=np.ones(6, bool))
    with pytest.raises(ValueError, match="pass the signed vector"):
        m.set_batch(1234, 5678, event=event, rows=5)
    m.set_batch(1234, 5678, rows=5)                                          # raw pointers are taken as they are
    assert m._yarg == 5678 and m.y is None


def test_family_of_and_the_family_lists_take_the_new_entry_and_keep_the_old():
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi import GammaReparamSVI, NegBinReparamSVI, WeibullReparamSVI
    assert mod.family_of(WeibullReparamSVI.__new__(WeibullReparamSVI)) == "weibull"
    assert mod.family_of(GammaReparamSVI.__new__(GammaReparamSVI)) == "gamma"
    assert mod.family_of(NegBinReparamSVI.__new__(NegBinReparamSVI)) == "negbin"
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}
