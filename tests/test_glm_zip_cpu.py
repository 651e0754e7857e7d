"""The float64 reference of the zero-inflated Poisson route (tests/_glm_zip_ref.py) checked against scipy and itself, what
a float32 pass can reach against the device bounds, and the driver's host side; no device needed.

Most of this file checks the REFERENCE and the bounds, not the product: it is what licenses EPS and the GPU tests'
yardstick.  The tests of the driver, of svi/predict.py's table and of the C ABI's symbols are the ones that fail
without the change.

 * log p against scipy.stats.poisson.logpmf composed with the mixture, rtol 1e-10; the predictive moments against the
   closed forms of the mixture;
 * d / d l and d / d tau against central differences of the reference's own log p per (row, draw); the tolerance is the
   difference between the quotients at h and h / 2;
 * the product form of a zero row's tau derivative equals sigmoid(u) - sigmoid(tau) and is never negative;
 * the device's link replayed step by step in float32 (tests/_glm_zip_ref.link_f32) within 1e-6 of the bound quantities
   at every shape tests/test_glm_zip_gpu.py runs (its two batches sized from the CU count at 256 CUs) and on a sample of
   l in [-12, 6] with 2 % in [-80, 80], tau in [-8, 8]; at l = +80 a zero row gives exactly log pi, 0 and 1 - pi;
 * EPS * bound below 1e-3 of the results at those shapes and seeds -- in the maximum norm over the draws of a statistic:
   T[s] changes sign in tau and is O(pi) at tau = -8 by construction, so a single draw's T can be arbitrarily small
   against its bound while the tolerance stays small against the scale of the vector the finish reads;
 * the constructor's refusals, each before a device is asked for, zero_share_mean against numerical integration, and the
   family tables."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.special import expit
from scipy.stats import poisson

import _glm_obs_ref as obs
import _glm_zip_ref as ref

F32_REACH = 1e-6        # what a plain float32 evaluation is held to, of the bound quantities (the device: ref.EPS = 2e-5)


def _mixture_logpmf(L, y, tau):
    """log( pi [y == 0] + (1 - pi) Poisson(y; e^l) ) from scipy's logpmf: [B, S]."""
    y64 = y.astype(np.float64)[:, None]
    t = tau.astype(np.float64)[None, :]
    lpi, l1m = -np.logaddexp(0.0, -t), -np.logaddexp(0.0, t)
    lp = l1m + poisson.logpmf(y64, np.exp(L))
    return np.where(y64 == 0, np.logaddexp(lpi, lp), lp)


def test_row_logpmf_is_scipys_poisson_composed_with_the_mixture():
    X, y, W, tau, o, _ = ref.make_inputs(300, 8, 6, 2, mode="offset")
    L = obs.logits(X, W, o)
    want = _mixture_logpmf(L, y, tau)
    npt.assert_allclose(ref.row_logpmf(L, y, tau), want, rtol=1e-10, atol=1e-12)
    assert 0.4 < (y == 0).mean() < 0.65 and (y >= 100).sum() > 10
    mu0 = np.exp(L[y == 0][:, 0])
    assert mu0.min() < 5e-3 and mu0.max() > 10.0                # zero rows pushed to small and large mu by the offset
    # ell is its sum without the row constant
    from scipy.special import gammaln
    ell, _, _ = ref.data_pass(X, y, W, tau, o, None)
    npt.assert_allclose(ell, (want + gammaln(y.astype(np.float64) + 1.0)[:, None]).sum(axis=0), rtol=1e-10)


def test_the_derivatives_of_log_p_in_l_and_tau():
    rs = np.random.RandomState(0)
    L = rs.uniform(-6.0, 3.5, (400, 5))
    tau = rs.uniform(-6.0, 6.0, (1, 5))
    y = np.where(rs.uniform(size=(400, 1)) < 0.5, 0.0, rs.poisson(3.0, (400, 1)) + 1.0)
    _, dl, dt = ref.link(L, y, tau)
    h = 2.0 ** -10
    for got, quotient in ((dl, lambda s: (ref.link(L + s, y, tau)[0] - ref.link(L - s, y, tau)[0]) / (2 * s)),
                          (dt, lambda s: (ref.link(L, y, tau + s)[0] - ref.link(L, y, tau - s)[0]) / (2 * s))):
        coarse, fine = quotient(h), quotient(h / 2)
        tol = np.abs(coarse - fine) + 1e-11
        assert (np.abs(got - fine) <= tol).all()
        assert (tol <= 1e-3 * np.maximum(np.abs(got), 1e-2)).all()          # the check is not vacuous
    zero = (y == 0)[:, 0]
    assert (dt[zero] >= 0).all() and (dt[~zero] < 0).all()


def test_the_zero_rows_tau_derivative_is_a_product_that_does_not_cancel():
    mu = np.exp(np.linspace(-80.0, 5.0, 500))[:, None]
    tau = np.linspace(-8.0, 8.0, 9)[None, :]
    _, _, dt = ref.link(np.log(mu), np.zeros((500, 1)), tau)
    diff = expit(tau + mu) - expit(tau)
    big = mu[:, 0] > 1e-3
    npt.assert_allclose(dt[big], diff[big], rtol=1e-12, atol=4e-16)   # (the difference carries two roundings of values <= 1)
    assert (dt > 0).all()                                       # e^{-80} included: the difference is 0 there in float64
    assert (diff[mu[:, 0] < 1e-20] == 0).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, tau, o, v = ref.make_inputs(60, 8, 4, 3)
    dead = y[v == 0]
    assert np.isnan(dead).any() and np.isinf(dead).any() and (dead < 0).any()
    keep = v > 0
    a = ref.data_pass(X, y, W, tau, o, v)
    b = ref.data_pass(X[keep], y[keep], W, tau, o[keep], v[keep])
    a32 = ref.data_pass_f32(X, y, W, tau, o, v)
    for p, q, p32 in zip(a, b, a32):
        assert np.isfinite(p).all() and np.isfinite(p32).all()
        npt.assert_allclose(p, q, rtol=1e-13, atol=1e-13 * np.abs(q).max())


def test_predictive_reference_against_the_mixtures_closed_forms():
    X, y, W, tau, o, _ = ref.make_inputs(150, 8, 16, 4, mode="offset")
    peak = np.abs(obs.logits(X, W, o)).max()
    W, o = (W * (3.0 / peak)).astype(np.float32), (o * (3.0 / peak)).astype(np.float32)
    L = obs.logits(X, W, o)
    out = ref.predict(X, W, tau, y, o)
    pi = expit(tau.astype(np.float64))[None, :]
    # moments of the mixture from the Poisson's: E y = (1 - pi) mu, E y^2 = (1 - pi)(mu + mu^2)
    mu = np.exp(L)
    m = (1.0 - pi) * mu
    var = (1.0 - pi) * (mu + mu * mu) - m * m
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-12)
    npt.assert_allclose(out["var"], var.mean(axis=1) + m.var(axis=1), rtol=1e-9)
    lp = _mixture_logpmf(L, y, tau)
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    npt.assert_allclose(np.exp(ref.predict(X, W, tau, np.zeros(150, np.float32), o)["lpd"]),
                        ref.zero_probability(X, W, tau, o), rtol=1e-12)
    b = ref.predict_bounds(X, W, tau, y, o)
    assert all((b[q] > 0).all() for q in ("mean", "var", "lpd")) and b["lpd_sum"] > 0


# ---- what float32 reaches ---------------------------------------------------------------------------------------------

def test_the_link_in_float32_on_a_sample_of_the_whole_range():
    """200 000 points, l in [-12, 6] with 2 % in [-80, 80], tau in [-8, 8], half of them zero rows: every term within
    1e-6 of its per-row bound quantity and no NaN."""
    rs = np.random.RandomState(11)
    n = 200000
    l = rs.uniform(-12.0, 6.0, n)
    wide = rs.uniform(size=n) < 0.02
    l[wide] = rs.uniform(-80.0, 80.0, wide.sum())
    tau = rs.uniform(-8.0, 8.0, n).astype(np.float32)
    y = np.where(rs.uniform(size=n) < 0.5, 0.0, rs.poisson(3.0, n) + 1.0).astype(np.float32)
    l = l.astype(np.float32)
    got = ref.link_f32(l, y, np.ones(n, np.float32), tau)
    l64, t64, y64 = (a.astype(np.float64) for a in (l, tau, y))
    lp, dl, dt = ref.link(l64, y64, t64)
    mu = np.exp(l64)
    b_ell = np.abs(t64) + mu + np.logaddexp(0.0, t64) + np.abs(y64 * l64) + 1.0
    b_T = np.abs(dt) + expit(t64) + 1.0
    b_r = y64 + mu + 1.0
    for g, w, b, name in zip(got, (lp, dl, dt), (b_ell, b_r, b_T), ("ell", "resid", "T")):
        assert np.isfinite(g).all(), name
        worst = float((np.abs(g - w) / b).max())
        print("float32 link, %s: worst error / bound quantity %.3g" % (name, worst))
        assert worst <= F32_REACH, (name, worst)
    assert (got[2][y == 0] >= 0).all()


def test_the_limits_of_the_link_in_float32():
    """l = +80 on a zero row: e^{-|u|} is 0, so log p = tau - L1 (log pi), d / d l = -mu 0 = 0 and d / d tau = 1 - pi,
    each exactly in the float32 values the launch holds; l = -80: finite, the closed forms to float32."""
    f = np.float32
    tau = np.linspace(-8.0, 8.0, 17).astype(f)
    L1 = np.logaddexp(0.0, tau.astype(np.float64)).astype(f)
    pi = expit(tau.astype(np.float64)).astype(f)
    one = np.ones(17, f)
    ell, r, T = ref.link_f32(np.full(17, 80.0, f), 0 * one, one, tau)
    npt.assert_array_equal(ell, tau - L1)
    npt.assert_allclose(ell, np.log(expit(tau.astype(np.float64))), atol=1e-6)
    assert (r == 0).all()
    npt.assert_array_equal(T, f(1.0) - pi)
    for yv in (0.0, 3.0):
        ell, r, T = ref.link_f32(np.full(17, -80.0, f), yv * one, one, tau)
        lp, dl, dt = ref.link(np.full(17, -80.0), np.full(17, yv), tau.astype(np.float64))
        assert np.isfinite(ell).all() and np.isfinite(r).all() and np.isfinite(T).all()
        npt.assert_allclose(ell, lp, rtol=2e-6, atol=2e-6)
        npt.assert_allclose(r, dl, rtol=1e-6, atol=1e-37)
        npt.assert_allclose(T, dt, rtol=1e-6, atol=1e-7)


def _ratios(X, y, W, tau, o, v):
    got = ref.data_pass_f32(X, y, W, tau, o, v)
    want = ref.data_pass(X, y, W, tau, o, v)
    bnd = ref.bounds(X, y, W, tau, o, v)
    assert all(np.isfinite(g).all() for g in got)
    reach = [float((np.abs(g - w) / b).max()) for g, w, b in zip(got, want, bnd)]
    # EPS * bound against the results, in the maximum norm over the draws (module docstring)
    hide = [float(ref.EPS * np.abs(b).max() / np.abs(w).max()) for w, b in zip(want, bnd)]
    return reach, hide


MI355X_CUS = 256      # tests/test_glm_zip_gpu.py sizes two batches from the device's CU count
TWO_TILES = [(MI355X_CUS * 4 * 16 * 2 + 5, 256, 8, "both", None, (), None),
             (MI355X_CUS * 4 * 8 * 2 + 3, 12, 8, "both", None, (), None)]


@pytest.mark.parametrize("B,D,S,mode,ld,shift,zeros", ref.PARITY_CASES + TWO_TILES)
def test_plain_float32_stays_inside_the_bounds_and_the_tolerance_hides_nothing(B, D, S, mode, ld, shift, zeros):
    X, y, W, tau, o, v = ref.make_inputs(B, D, S, seed=ref.case_seed(B, D, S), mode=mode, zeros=zeros)
    reach, hide = _ratios(X, y, W, tau, o, v)
    print("B=%d D=%d S=%d %s zeros=%s: error / bound quantity ell %.3g, G %.3g, T %.3g; EPS * bound / result ell %.3g, "
          "G %.3g, T %.3g" % ((B, D, S, mode, zeros) + tuple(reach) + tuple(hide)))
    assert max(reach) <= F32_REACH
    assert max(hide) <= 1e-3
    keep = np.ones(B, bool) if v is None else v > 0
    share = (y[keep] == 0).mean()
    assert share == zeros if zeros in (0.0, 1.0) else 0.4 < share < 0.65
    assert ref.TAU_LO <= tau.min() and tau.max() <= ref.TAU_HI


def test_the_recorded_figures_of_the_end_to_end_fit_are_the_reference_drivers():
    """tests/test_glm_zip_gpu.py's end-to-end test holds the device to tests/_glm_zip_ref.E2E_REF: these are what the
    float64 reference driver ends at, and it has found the simulated share and intercept to two of its own standard
    deviations."""
    c, r = ref.E2E, ref.E2E_REF
    X, y = ref.simulate(c["B"], c["D"], c["seed"])
    n, D = c["fit_rows"], c["D"]
    lam = ref.fit(X[:n], y[:n], c["S"], c["vi_seed"], c["steps"], c["lr"], c["prec"], c["a0"], c["b0"])
    sd = np.exp(lam[D + 1:])
    npt.assert_allclose([lam[0], sd[0], lam[D], sd[D]], [r["intercept"], r["intercept_sd"], r["tau"], r["tau_sd"]],
                        atol=1e-5)
    npt.assert_allclose(ref.zero_share_mean(lam[D], sd[D] ** 2), r["zero_share"], atol=1e-5)
    assert abs(r["zero_share"] - 0.3) < 2.0 * r["zero_share"] * (1.0 - r["zero_share"]) * r["tau_sd"]
    assert abs(r["intercept"] - math.log(2.0)) < 2.0 * r["intercept_sd"]
    assert 0.35 < (y[:n] == 0).mean() < 0.45


# ---- the driver's host side ---------------------------------------------------------------------------------------------

def test_constructor_refusals_need_no_device():
    from bayesic_amd.svi import ZIPoissonReparamSVI
    X = np.zeros((5, 4), np.float32)
    y = np.arange(5, dtype=np.float32)
    for wrong in (0.5, -1.0, np.nan, np.inf):
        bad = y.copy()
        bad[2] = wrong
        with pytest.raises(ValueError, match="y must be finite, >= 0 and whole"):
            ZIPoissonReparamSVI(X, bad)
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        ZIPoissonReparamSVI(X, y, lam0=np.zeros(8))
    with pytest.raises(ValueError, match="covariance"):
        ZIPoissonReparamSVI(X, y, covariance="nope")
    for a0 in (0.0, -1.0):
        with pytest.raises(ValueError, match="a0 and b0"):
            ZIPoissonReparamSVI(X, y, a0=a0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        ZIPoissonReparamSVI(X, y, n_samples=65)
    with pytest.raises(ValueError, match="exposure and offset are mutually exclusive"):
        ZIPoissonReparamSVI(X, y, offset=np.zeros(5, np.float32), exposure=np.ones(5, np.float32))
    with pytest.raises(TypeError):
        ZIPoissonReparamSVI(X, y, upper=np.full(5, np.inf, np.float32))      # there are no upper ends


def test_the_default_prior_mean_of_the_odds_is_one():
    import inspect
    from bayesic_amd.svi import NegBinReparamSVI, ZIPoissonReparamSVI
    sig = inspect.signature(ZIPoissonReparamSVI.__init__).parameters
    assert sig["a0"].default / sig["b0"].default == 1.0
    nb = inspect.signature(NegBinReparamSVI.__init__).parameters
    assert nb["a0"].default / nb["b0"].default == 10.0                       # the other families' default stays
    assert "91 %" in ZIPoissonReparamSVI.__init__.__doc__


def test_set_batch_checks_y_and_params_report_the_zero_share():
    import torch
    from bayesic_amd.svi import ZIPoissonReparamSVI
    from bayesic_amd.svi._reparam_base import unpack_full
    m = ZIPoissonReparamSVI.__new__(ZIPoissonReparamSVI)
    m.D, m.ctx = 4, None
    X = torch.zeros((5, 4))
    m.set_batch(X, torch.tensor([0.0, 1.0, 0.0, 7.0, 2.0]))
    assert m.B == 5 and m.offset is None and m.weights is None
    for wrong in (0.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="y must be finite, >= 0 and whole"):
            m.set_batch(X, torch.tensor([0.0, 1.0, wrong, 7.0, 2.0]))
    m.set_batch(1234, 5678, rows=5)                                          # raw pointers are taken as they are
    assert m._yarg == 5678 and m.y is None
    D = 4
    for m_tau, sd in ((0.7, 0.3), (-2.0, 1.5), (3.0, 0.05)):
        m.covariance_kind = "diag"
        lam = np.concatenate([[0.1, 0.2, 0.3, 0.4, m_tau], np.log([0.1, 0.1, 0.1, 0.1, sd])])
        m._lam, m.t = torch.from_numpy(lam)[None, :], 0
        p = m.params()
        npt.assert_allclose(p["odds_mean"], math.exp(m_tau + 0.5 * sd * sd), rtol=1e-12)
        npt.assert_allclose(p["zero_share_mean"], ref.zero_share_mean(m_tau, sd * sd), rtol=1e-9)
        assert abs(p["zero_share_mean"] - float(expit(m_tau))) > 1e-6 or sd < 0.1    # not the plug-in value
    # the full guide: the marginal variance of tau is the squared norm of the whole last row of L
    m.covariance_kind = "full"
    P = D + 1
    rs = np.random.RandomState(0)
    lam_full = np.concatenate([lam[:P], 0.4 * rs.standard_normal(P * (P + 1) // 2)])
    m._lam = torch.from_numpy(lam_full)[None, :]
    L = unpack_full(lam_full, P)[1]
    var = float((L[D] ** 2).sum())
    assert var > 2.0 * L[D, D] ** 2 or var > 0.1
    npt.assert_allclose(m.params()["zero_share_mean"], ref.zero_share_mean(lam_full[D], var), rtol=1e-9)


def test_family_of_and_the_family_lists_take_the_new_entry_and_keep_the_old():
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi import NegBinReparamSVI, ZIPoissonReparamSVI
    assert mod.family_of(ZIPoissonReparamSVI.__new__(ZIPoissonReparamSVI)) == "zip"
    assert mod.family_of(NegBinReparamSVI.__new__(NegBinReparamSVI)) == "negbin"
    row = mod.FAMILY_TABLE["zip"]
    assert row.entry == "bsc_zip_predict_pass" and row.scalar and row.grouped is None
    assert row.link not in ("log", "logit", "location", None)                # a word of its own
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.LOGIT_SCALAR_PASSES == {"beta": "bsc_beta_predict_pass"}
    assert mod.SCALAR_FAMILIES == {"negbin": 0, "gamma": 1, "weibull": 2}
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}
    assert ZIPoissonReparamSVI.link == "zip" and ZIPoissonReparamSVI.mean_key == "odds_mean"
    assert ZIPoissonReparamSVI.has_exposure is True


def test_the_c_abi_has_the_three_entry_points_with_the_shared_signatures():
    from bayesic_amd import _ffi
    for name, twin in (("bsc_glm_zip_data_pass", "bsc_glm_nb_data_pass"), ("bsc_glm_zip_update", "bsc_glm_nb_update"),
                       ("bsc_zip_predict_pass", "bsc_nb_predict_pass")):
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[twin]
        assert _ffi.SIGNATURES[name] is not _ffi.SIGNATURES[twin]


def test_predict_takes_exposure_as_a_log_link_and_refuses_upper_and_groups_before_a_device_is_asked_for():
    from bayesic_amd.svi import ZIPoissonReparamSVI
    from bayesic_amd.svi import predict as mod
    m = ZIPoissonReparamSVI.__new__(ZIPoissonReparamSVI)
    m.D, m.ctx = 4, None
    X = np.zeros((5, 4), np.float32)
    y = np.ones(5, np.float32)
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not zip"):
        mod.predict(m, X, y, upper=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, groups=np.zeros(5, np.int32))
    # a log link: offset and exposure together are refused in the Poisson model's words (exposure alone is taken:
    # tests/test_glm_zip_gpu.py)
    with pytest.raises(ValueError, match="exposure and offset are mutually exclusive"):
        mod.predict(m, X, y, offset=np.zeros(5, np.float32), exposure=np.ones(5, np.float32))
    m.has_offset = True
    with pytest.raises(ValueError, match="fitted with an offset"):
        mod.predict(m, X, y)
