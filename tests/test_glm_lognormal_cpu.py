"""The float64 reference of the log-normal survival route (tests/_glm_lognormal_ref.py) checked against scipy and itself,
what a float32 pass can reach against the device bounds, and the driver's host side; no device needed.

Most of this file checks the REFERENCE and the bounds, not the product: it is what licenses EPS and the GPU tests'
yardstick, and those tests pass whether or not the feature is built.  The tests of the driver, of svi/predict.py's tables
and of the special function's coefficients (read from csrc/bsc_special_f32.h) are the ones that fail without the change.

 * log f and log S against scipy.stats.lognorm.logpdf and .logsf (s = sigma, scale = e^l), rtol 1e-10;
 * G and T against central differences of the reference's own ell in w and tau on a batch of events and censored rows;
   the tolerance is the difference between the quotients at h and h / 2 (three times the finer one's truncation error);
 * every row an event: ell is the Gaussian log-density of log t minus sum v log t, in closed form;
 * a censored-only batch has every residual > 0; a zero-weight row holding 0 or NaN changes nothing;
 * the predictive moments against lognorm.mean and .var, survival against the draw average of lognorm.sf; the moment
   factors fit float32 at the lower end of the envelope and not at tau = -2;
 * the device's erfcx replayed in float32 with the header's own coefficients, within 1.8 roundings of scipy's erfcx over
   [0, 1e19]; the special function built on it within 8 float32 roundings of its own results over z in [-60, 60];
 * the device's forms in plain float32 (data_pass_f32, on that replay) within 1e-6 of the bound quantities at every shape
   tests/test_glm_lognormal_gpu.py runs (its two batches sized from the CU count at 256 CUs), at the corners of the
   envelope, tau in {-1.5, 4} with z from -60 to 60, and at z = +-60 pinned;
 * the constructor's refusals, each before a device is asked for, and the family tables."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.stats import lognorm

import _glm_obs_ref as obs
import _glm_lognormal_ref as ref

F32_REACH = 1e-6        # what a plain float32 evaluation is held to, of the bound quantities (the device: ref.EPS = 2e-5)


def test_row_logpdf_is_scipys_lognormal_density_and_survival():
    X, y, W, lis, o, _ = ref.make_inputs(200, 8, 6, 2, mode="offset")
    L = obs.logits(X, W, o)
    sigma = np.exp(-lis.astype(np.float64))[None, :]
    t = np.abs(y.astype(np.float64))[:, None]
    event = (y > 0)[:, None]
    want = np.where(event, lognorm.logpdf(t, sigma, scale=np.exp(L)), lognorm.logsf(t, sigma, scale=np.exp(L)))
    npt.assert_allclose(ref.row_logpdf(L, y, lis), want, rtol=1e-10)
    assert 40 < (y < 0).sum() < 80 and lis.min() == ref.TAU_LO and lis.max() == ref.TAU_HI
    # and ell is its sum: nothing is left out
    ell, _, _ = ref.data_pass(X, y, W, lis, o, None)
    npt.assert_allclose(ell, want.sum(axis=0), rtol=1e-10)


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 60, 4, 3
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, 1, z_max=3.0, tau=[-1.0, 0.25, 1.25])
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)       # w +- h and tau +- h exact in float32
    W, lis = q(W), q(lis)
    assert (y[v > 0] > 0).any() and (y[v > 0] < 0).any()
    _, G, T = ref.data_pass(X, y, W, lis, o, v)
    b_ell = ref.bounds(X, y, W, lis, o, v)[0]

    def quotient(s, d, h):
        Wp, Wm, tp, tm = W.copy(), W.copy(), lis.copy(), lis.copy()
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


def test_with_every_row_an_event_ell_is_the_gaussian_density_of_log_t():
    X, y, W, lis, o, v = ref.make_inputs(120, 8, 4, 3, censored=0.0)
    keep = v > 0
    assert (y[keep] > 0).all()
    ell, G, T = ref.data_pass(X, y, W, lis, o, v)
    ly = np.log(y[keep].astype(np.float64))
    vk = v[keep].astype(np.float64)
    L = obs.logits(X, W, o)[keep]
    for s in range(4):
        tau = float(lis[s])
        res = ly - L[:, s]
        want = (vk * (tau - 0.5 * ref.LOG_2PI - 0.5 * math.exp(2.0 * tau) * res * res)).sum() - (vk * ly).sum()
        npt.assert_allclose(ell[s], want, rtol=1e-12)
        # the normal equations: G = k^2 sum v res x, T = sum v (1 - k^2 res^2)
        npt.assert_allclose(G[s], math.exp(2.0 * tau) * (vk * res) @ X[keep].astype(np.float64), rtol=1e-10, atol=1e-9)
        npt.assert_allclose(T[s], (vk * (1.0 - math.exp(2.0 * tau) * res * res)).sum(), rtol=1e-12)


def test_a_censored_only_batch_pushes_every_location_up():
    X, y, W, lis, o, v = ref.make_inputs(90, 8, 5, 4, censored=1.0, z_max=8.0)    # (at z = -40 the hazard is 0 in float64)
    assert (y[v > 0] < 0).all()
    r = ref._terms(X, y, W, lis, o, v)[2]
    assert (r >= 0).all() and (r[v > 0] > 0).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, lis, o, v = ref.make_inputs(40, 8, 4, 3)
    v[36:] = 0.0
    y[36:] = [0.0, np.nan, np.inf, -0.0]
    o[36:] = [200.0, -1.0e30, 1.0e30, 0.0]
    keep = v > 0
    a = ref.data_pass(X, y, W, lis, o, v)
    b = ref.data_pass(X[keep], y[keep], W, lis, o[keep], v[keep])
    a32 = ref.data_pass_f32(X, y, W, lis, o, v)
    for p, q, p32 in zip(a, b, a32):
        assert np.isfinite(p).all() and np.isfinite(p32).all()
        npt.assert_allclose(p, q, rtol=1e-13, atol=1e-13 * np.abs(q).max())
    assert (v == 0).sum() >= 10 and np.isnan(y[v == 0]).any() and (y[v == 0] == 0).any()


def test_predictive_reference_against_scipy():
    B, D, S = 120, 8, 16
    X, y, W, lis, o, _ = ref.make_inputs(B, D, S, 4, mode="offset")
    out = ref.predict(X, W, lis, y, o)
    L = obs.logits(X, W, o)
    sigma = np.exp(-lis.astype(np.float64))[None, :]
    m = lognorm.mean(sigma, scale=np.exp(L))
    v = lognorm.var(sigma, scale=np.exp(L))
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-10)
    npt.assert_allclose(out["var"], v.mean(axis=1) + m.var(axis=1), rtol=1e-8)       # law of total variance
    t = np.abs(y.astype(np.float64))[:, None]
    lp = np.where((y > 0)[:, None], lognorm.logpdf(t, sigma, scale=np.exp(L)), lognorm.logsf(t, sigma, scale=np.exp(L)))
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    # survival: the draw average of scipy's sf, and exp(lpd) of the batch with every row censored
    npt.assert_allclose(ref.survival(X, W, lis, t[:, 0], o), lognorm.sf(t, sigma, scale=np.exp(L)).mean(axis=1),
                        rtol=1e-10, atol=1e-300)
    npt.assert_allclose(np.exp(ref.predict(X, W, lis, -t[:, 0], o)["lpd"]), ref.survival(X, W, lis, t[:, 0], o),
                        rtol=1e-10, atol=1e-300)
    b = ref.predict_bounds(X, W, lis, y, o)
    assert all((b[q] > 0).all() for q in ("mean", "var", "lpd")) and b["lpd_sum"] > 0


def test_the_moment_factors_fit_float32_at_the_lower_end_of_the_envelope_and_not_below_it():
    """The variance factor (e^{sigma^2} - 1) e^{sigma^2} is what sets TAU_LO: 2.8e17 at tau = -1.5, leaving e^{2l} room up
    to l = 24; at tau = -2 (sigma^2 = 54.6) it is e^{109}, beyond the float32 maximum e^{88.7}."""
    fmax = float(np.finfo(np.float32).max)
    m1, m2 = ref.moment_constants(ref.TAU_LO)
    assert m1 < m2 < 1e18 and m2 * math.exp(2.0 * 20.0) < fmax
    assert ref.moment_constants(-2.0)[1] > fmax
    m1, m2 = ref.moment_constants(ref.TAU_HI)
    assert abs(m1 - 1.0) < 2e-4 and 3e-4 < m2 < 4e-4 and np.float32(m2) > 0


# ---- what float32 reaches ---------------------------------------------------------------------------------------------

def test_the_devices_erfcx_replayed_in_float32_with_the_headers_coefficients():
    """tests/_glm_lognormal_ref.erfcx_pos_f32 is csrc/bsc_special_f32.h's bsc_erfcx_pos_f32 step by step; its twelve
    coefficients are the ones the header holds, in the header's order.  The header states 1.8 float32 roundings of erfcx
    over [0, 1e19]: the polynomial's own 1.9e-8 is a sixth of a rounding of a result in [0.1, 1], each of the two
    corrected quotients costs one rounding at most and the closing fmaf half of one."""
    import pathlib
    import re
    from scipy.special import erfcx
    text = (pathlib.Path(__file__).resolve().parent.parent / "bayesic_amd" / "csrc" / "bsc_special_f32.h").read_text()
    body = text[text.index("float bsc_erfcx_pos_f32(float a) {"):text.index("// The log survival function")]
    lead = re.findall(r"float p = (-?[0-9.e+-]+)f;", body)
    rest = re.findall(r"p = fmaf\(p, t, (-?[0-9.e+-]+)f\);", body)
    assert [float(c) for c in lead + rest] == list(ref.ERFCX_COEF)
    a = np.concatenate([np.linspace(0.0, 6.0, 400001), np.linspace(6.0, 60.0, 200001),
                        np.geomspace(60.0, 1e19, 20001)]).astype(np.float32)
    got = ref.erfcx_pos_f32(a)
    want = erfcx(a.astype(np.float64))
    assert np.isfinite(got).all() and (got > 0).all() and (got <= 1).all()
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print("erfcx replay: worst %.2f roundings at a = %.4g" % (ulp.max(), a[ulp.argmax()]))
    assert ulp.max() <= 1.8


def test_the_special_function_in_float32_stays_within_a_few_roundings():
    """csrc/bsc_special_f32.h's forms in float32 arithmetic over z in [-60, 60] and around 0, each result against ITSELF
    in float64.  At most eight rounded operations stand between z and either result (the scaled argument, E, the square,
    the exponential, its correction, q, the logarithm and the closing fmaf; for the hazard a reciprocal and two products
    in place of the last two), each a rounding of a quantity no larger than the result's own size and none amplified by
    more than 1.5 (log1p(-q) against q at q = 1/2): both are held to 8 roundings.  Measured here: 2.8 and 2.6, both on
    the left at |z| near 1.  Nothing overflows, the hazard runs to 0 on the left and log Phi(-z) to -0."""
    z = np.concatenate([np.linspace(-60.0, 60.0, 240001), np.linspace(-1e-3, 1e-3, 2001),
                        [-60.0, 60.0, 0.0, -0.0]]).astype(np.float32)
    lsf, h = ref.log_sf_hazard_f32(z)
    lsf_r, h_r = ref.log_sf_hazard(z.astype(np.float64))
    eps = float(np.finfo(np.float32).eps)
    assert np.isfinite(lsf).all() and np.isfinite(h).all()
    e_lsf = np.abs(lsf - lsf_r) / (eps * np.abs(lsf_r) + float(np.finfo(np.float32).tiny))
    e_h = np.abs(h - h_r) / (eps * h_r + float(np.finfo(np.float32).tiny))
    print("float32 forms: log Phi(-z) within %.2f roundings, hazard within %.2f" % (e_lsf.max(), e_h.max()))
    assert e_lsf.max() <= 8.0 and e_h.max() <= 8.0
    assert h[z == -60.0][0] == 0.0 and abs(lsf[z == 60.0][0] + 1805.0135) < 1e-3 and lsf[z == -60.0][0] == 0.0


def _f32_ratios(X, y, W, lis, o, v):
    got = ref.data_pass_f32(X, y, W, lis, o, v)
    want = ref.data_pass(X, y, W, lis, o, v)
    bnd = ref.bounds(X, y, W, lis, o, v)
    assert all(np.isfinite(g).all() for g in got)
    return [float((np.abs(g - w) / b).max()) for g, w, b in zip(got, want, bnd)]


MI355X_CUS = 256      # tests/test_glm_lognormal_gpu.py sizes two batches from the device's CU count

GPU_SHAPES = [(1003, 12, 8), (517, 200, 11), (1003, 256, 3), (1029, 256, 8), (1029, 256, 11),
              (MI355X_CUS * 4 * 16 * 2 + 5, 256, 8), (MI355X_CUS * 4 * 8 * 2 + 3, 12, 8)]


@pytest.mark.parametrize("B,D,S,censored", [s + (0.3,) for s in GPU_SHAPES] + [(1003, 12, 8, 0.0), (1003, 12, 8, 1.0)])
def test_plain_float32_stays_inside_the_bounds_at_the_gpu_shapes(B, D, S, censored):
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, censored=censored)
    r_ell, r_G, r_T = _f32_ratios(X, y, W, lis, o, v)
    print("B=%d D=%d S=%d censored %.1f: error / bound quantity ell %.3g, G %.3g, T %.3g" % (
        B, D, S, censored, r_ell, r_G, r_T))
    assert max(r_ell, r_G, r_T) <= F32_REACH
    assert ref.TAU_LO <= lis.min() and lis.max() <= ref.TAU_HI


@pytest.mark.parametrize("tau", [ref.TAU_LO, ref.TAU_HI])
def test_plain_float32_stays_inside_the_bounds_at_the_corners_of_the_envelope(tau):
    """z from -60 to 60 at log t in {-80, -5, 0, 5, 80}; the logit is l = log t - z / k, almost all of it through the
    offset: |l| reaches 80 + 60 / k, about 350 at tau = -1.5 (the pass never forms e^l)."""
    rs = np.random.RandomState(7)
    B, D, S = 640, 8, 2
    k = math.exp(tau)
    z = np.tile(np.linspace(-60.0, 60.0, B // 5), 5)
    ly = np.repeat([-80.0, -5.0, 0.0, 5.0, 80.0], B // 5)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.01 / max(k, 1.0) * rs.standard_normal((S, D))).astype(np.float32)
    o = (ly - z / k).astype(np.float32)
    y = np.exp(ly).astype(np.float32)
    y[rs.uniform(size=B) < 0.3] *= -1.0
    v = rs.uniform(0.5, 2.0, B).astype(np.float32)
    lis = np.full(S, tau, np.float32)
    z_real = k * (np.log(np.abs(y.astype(np.float64)))[:, None] - obs.logits(X, W, o))
    assert 59.0 < z_real.max() < 61.0 and -61.0 < z_real.min() < -59.0 and np.abs(o).max() > 80.0 + 59.0 / k
    r_ell, r_G, r_T = _f32_ratios(X, y, W, lis, o, v)
    print("tau=%g: error / bound quantity ell %.3g, G %.3g, T %.3g" % (tau, r_ell, r_G, r_T))
    assert max(r_ell, r_G, r_T) <= F32_REACH


def test_plain_float32_stays_inside_the_bounds_with_z_pinned_at_plus_and_minus_60():
    X, y, W, lis, o, v = ref.make_pinned(1003, 12, 8, 3)
    z = math.exp(float(lis[0])) * (np.log(np.abs(y.astype(np.float64))) - obs.logits(X, W, o)[:, 0])
    assert (y < 0).all() and (np.abs(np.abs(z) - 60.0) < 1e-3).all() and (z > 0).any() and (z < 0).any()
    r_ell, r_G, r_T = _f32_ratios(X, y, W, lis, o, v)
    print("z = +-60: error / bound quantity ell %.3g, G %.3g, T %.3g" % (r_ell, r_G, r_T))
    assert max(r_ell, r_G, r_T) <= F32_REACH


# ---- the driver's host side ---------------------------------------------------------------------------------------------

def test_constructor_refusals_need_no_device():
    from bayesic_amd.svi import LogNormalReparamSVI
    X = np.zeros((5, 4), np.float32)
    time = np.arange(1, 6, dtype=np.float32)
    for wrong in (0.0, -1.0, np.nan, np.inf):
        bad = time.copy()
        bad[2] = wrong
        with pytest.raises(ValueError, match="time must be finite and > 0"):
            LogNormalReparamSVI(X, bad)
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        LogNormalReparamSVI(X, time, np.ones(4, bool))
    with pytest.raises(ValueError, match="event must be a bool or 0/1 array of length 5"):
        LogNormalReparamSVI(X, time, event=np.array([0, 1, 2, 0, 1]))
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        LogNormalReparamSVI(X, time, lam0=np.zeros(8))
    with pytest.raises(ValueError, match="covariance"):
        LogNormalReparamSVI(X, time, covariance="nope")
    with pytest.raises(ValueError, match="a0 and b0"):
        LogNormalReparamSVI(X, time, a0=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        LogNormalReparamSVI(X, time, n_samples=65)
    with pytest.raises(TypeError):
        LogNormalReparamSVI(X, time, exposure=np.ones(5, np.float32))        # there is no exposure keyword
    with pytest.raises(TypeError):
        LogNormalReparamSVI(X, time, upper=np.full(5, np.inf, np.float32))   # and no upper ends


def test_set_batch_packs_the_signed_vector_and_params_report_both_means():
    import torch
    from bayesic_amd.svi.glm_lognormal import LogNormalReparamSVI
    from bayesic_amd.svi.glm_weibull import pack_response
    import bayesic_amd.svi.glm_lognormal as mod
    assert mod.pack_response is pack_response                                # imported, not copied
    time = np.array([0.5, 2.0, 3.0, 4.0, 1.0e-3], np.float32)
    event = np.array([1, 0, 1, 0, 0])
    want = np.array([0.5, -2.0, 3.0, -4.0, -1.0e-3], np.float32)
    m = LogNormalReparamSVI.__new__(LogNormalReparamSVI)
    m.D, m.ctx = 4, None
    X = torch.zeros((5, 4))
    m.set_batch(X, torch.from_numpy(time), event=event)
    npt.assert_array_equal(m.y.numpy(), want)
    assert m._yarg is m.y and m.B == 5 and m.offset is None and m.weights is None
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        m.set_batch(X, torch.from_numpy(-time))
    with pytest.raises(TypeError):
        m.set_batch(X, torch.from_numpy(time), upper=torch.ones(5))
    with pytest.raises(ValueError, match="pass the signed vector"):
        m.set_batch(1234, 5678, event=event, rows=5)
    m.set_batch(1234, 5678, rows=5)                                          # raw pointers are taken as they are
    assert m._yarg == 5678 and m.y is None
    # params(): E_q[e^tau] and E_q[e^{-tau}], mean-field and full (the marginal variance of tau: the whole last row of L)
    D = 4
    m.covariance_kind = "diag"
    lam = np.concatenate([[0.1, 0.2, 0.3, 0.4, 0.7], np.log([0.1, 0.1, 0.1, 0.1, 0.3])])
    m._lam, m.t = torch.from_numpy(lam)[None, :], 0
    p = m.params()
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(0.7 + 0.045), rtol=1e-12)
    npt.assert_allclose(p["sigma_mean"], math.exp(-0.7 + 0.045), rtol=1e-12)
    from bayesic_amd.svi._reparam_base import unpack_full
    m.covariance_kind = "full"
    P = D + 1
    rs = np.random.RandomState(0)
    lam_full = np.concatenate([lam[:P], 0.1 * rs.standard_normal(P * (P + 1) // 2)])
    m._lam = torch.from_numpy(lam_full)[None, :]
    L = unpack_full(lam_full, P)[1]
    var = float((L[D] ** 2).sum())
    p = m.params()
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(0.7 + 0.5 * var), rtol=1e-12)
    npt.assert_allclose(p["sigma_mean"], math.exp(-0.7 + 0.5 * var), rtol=1e-12)


def test_family_of_and_the_family_lists_take_the_new_entry_and_keep_the_old():
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi import LogNormalReparamSVI, WeibullReparamSVI
    assert mod.family_of(LogNormalReparamSVI.__new__(LogNormalReparamSVI)) == "lognormal"
    assert mod.family_of(WeibullReparamSVI.__new__(WeibullReparamSVI)) == "weibull"
    assert mod.FAMILY_TABLE["lognormal"].entry == "bsc_lognormal_predict_pass"
    assert mod.FAMILY_TABLE["lognormal"].scalar and mod.FAMILY_TABLE["lognormal"].grouped is None
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.LOGIT_SCALAR_PASSES == {"beta": "bsc_beta_predict_pass"}
    assert mod.SCALAR_FAMILIES == {"negbin": 0, "gamma": 1, "weibull": 2}
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}


def test_predict_refuses_exposure_upper_and_groups_before_a_device_is_asked_for():
    from bayesic_amd.svi import LogNormalReparamSVI
    from bayesic_amd.svi import predict as mod
    m = LogNormalReparamSVI.__new__(LogNormalReparamSVI)
    m.D, m.ctx = 4, None
    X = np.zeros((5, 4), np.float32)
    y = np.ones(5, np.float32)
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not lognormal"):
        mod.predict(m, X, y, upper=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, groups=np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the lognormal model takes offset="):
        mod.predict(m, X, y, exposure=np.ones(5, np.float32))
