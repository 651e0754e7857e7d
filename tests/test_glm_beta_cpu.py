"""The float64 reference of the Beta route (tests/_glm_beta_ref.py) checked against scipy and itself, what a float32 pass
can reach against the device bounds, the driver's refusals, and the recovery run of tests/test_glm_beta_gpu.py in the
reference alone; no device needed.

 * the per-row log density against scipy.stats.beta.logpdf(y, m phi, (1 - m) phi), rtol 1e-9;
 * G and T against central differences of the reference's own ell in w and tau;
 * at m = 1/2, phi = 2 the density is uniform: ell = 0 exactly;
 * data_pass_f32 -- the kernel's formulas (csrc/bsc_glm_pass.h's GLM_BETA link over csrc/bsc_special_f32.h's
   bsc_lgamma_psi_f32) in plain float32 numpy -- below 1e-6 of b_ell, b_T and max|G| on make_inputs across tau in [-2, 5]
   and on the +-80 / +-70 logits of make_extreme_inputs, every term finite: the headroom the tolerances of
   tests/test_glm_beta_gpu.py (2e-5 and 1e-4) lean on;
 * lgamma_psi_f32 itself against scipy from 1e-36 to 200;
 * the predictive against scipy's mean, variance and logpdf;
 * the driver's argument errors that are raised before a device is asked for, and svi/predict.py's pinned tables;
 * the reference stepper on the recovery data: precision_mean within 15 % of the true 20, which licenses that bound in
   the GPU test."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.special import digamma, expit, gammaln
from scipy.stats import beta as beta_dist

import _glm_beta_ref as ref
import _glm_obs_ref as obs


def _small(B, D, S, seed):
    """Inputs on a grid of 2^-12 so that w +- 2^-10 and tau +- 2^-10 are exact float32 values."""
    X, y, W, logprec, o, v = ref.make_inputs(B, D, S, seed)
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)
    return X, y, q(W), q(logprec), o, v


def test_row_logpdf_is_scipys_beta():
    X, y, W, logprec, o, _ = ref.make_inputs(200, 8, 6, 2)
    L = obs.logits(X, W, o)
    phi = np.exp(logprec.astype(np.float64))[None, :]
    want = beta_dist.logpdf(y.astype(np.float64)[:, None], expit(L) * phi, expit(-L) * phi)
    npt.assert_allclose(ref.row_logpdf(L, y, logprec), want, rtol=1e-9, atol=1e-12)
    assert y.min() == np.float32(1e-6) and y.max() == np.float32(1.0 - 1e-6)
    assert logprec.min() < 0.0 < 2.0 < logprec.max()
    # and ell is its sum: nothing is left out
    ell, _, _ = ref.data_pass(X, y, W, logprec, o, None)
    npt.assert_allclose(ell, want.sum(axis=0), rtol=1e-9)


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 60, 4, 3
    X, y, W, logprec, o, v = _small(B, D, S, 1)
    ell, G, T = ref.data_pass(X, y, W, logprec, o, v)
    h = 2.0 ** -10
    for s in range(S):
        for d in range(D):
            Wp, Wm = W.copy(), W.copy()
            Wp[s, d] += h
            Wm[s, d] -= h
            fd = (ref.data_pass(X, y, Wp, logprec, o, v)[0][s] - ref.data_pass(X, y, Wm, logprec, o, v)[0][s]) / (2 * h)
            npt.assert_allclose(G[s, d], fd, rtol=1e-4, atol=1e-4 * np.abs(G).max())
        tp, tm = logprec.copy(), logprec.copy()
        tp[s] += h
        tm[s] -= h
        fd = (ref.data_pass(X, y, W, tp, o, v)[0][s] - ref.data_pass(X, y, W, tm, o, v)[0][s]) / (2 * h)
        npt.assert_allclose(T[s], fd, rtol=1e-4, atol=1e-4 * np.abs(T).max())
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_uniform_density_at_half_and_precision_two_is_exactly_zero():
    """m = 1/2, phi = 2: a = b = 1, Beta(1, 1) is the uniform density on (0, 1) and every term of its logarithm is an
    exact zero (lnGamma(2) = lnGamma(1) = 0, a - 1 = b - 1 = 0), for every y and every weight."""
    y = np.array([1e-6, 0.25, 0.5, 0.75, 1.0 - 1e-6], np.float32)
    v = np.array([0.5, 1.0, 2.0, 0.0, 3.0])
    lp = ref.row_logpdf(np.zeros((5, 1)), y, None, phi=[2.0])          # phi = 2 itself: no float32 tau has e^tau = 2
    npt.assert_array_equal(lp, np.zeros((5, 1)))
    assert (v @ lp)[0] == 0.0                                           # ell, whatever the weights
    # through tau = log 2 rounded to float32 (what a pass reads) phi is 2 (1 + 2e-9) and ell is zero to that
    X, W = np.eye(5, 8, dtype=np.float32), np.zeros((1, 8), np.float32)
    tau = np.array([math.log(2.0)], np.float32)
    ell, G, T = ref.data_pass(X, y, W, tau, None, v.astype(np.float32))
    b_ell, _ = ref.bounds(X, y, W, tau, None, v.astype(np.float32))
    assert abs(ell[0]) <= 1e-9 * b_ell[0]
    # G is v phi / 4 (log y - log1p(-y)): zero at y = 1/2 alone (row 3 has weight 0)
    assert G[0, 2] == 0.0 and G[0, 3] == 0.0 and G[0, 0] < 0.0 < G[0, 4]
    assert np.isfinite(T).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, logprec, o, v = ref.make_inputs(40, 8, 4, 3)
    v[35:] = 0.0
    y[35:] = [0.0, 1.0, 2.0, np.nan, 1.0e30]
    o[35:] = [200.0, -1.0e30, 1.0e30, 0.0, -200.0]
    a = ref.data_pass(X, y, W, logprec, o, v)
    b = ref.data_pass(X[:35], y[:35], W, logprec, o[:35], v[:35])
    for p, q in zip(a, b):
        assert np.isfinite(p).all()
        npt.assert_array_equal(p, q)


def _f32_ratios(X, y, W, logprec, o, v):
    ell, G, T = ref.data_pass_f32(X, y, W, logprec, o, v)
    ell_r, G_r, T_r = ref.data_pass(X, y, W, logprec, o, v)
    b_ell, b_T = ref.bounds(X, y, W, logprec, o, v)
    assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(T).all()
    return ((np.abs(ell - ell_r) / b_ell).max(), (np.abs(T - T_r) / b_T).max(),
            np.abs(G - G_r).max() / np.abs(G_r).max())


@pytest.mark.parametrize("B,D,S", [(37, 64, 11), (165, 252, 11), (325, 256, 11), (1003, 256, 8)])
def test_plain_float32_stays_below_1e_6_of_the_bound_quantities(B, D, S):
    """tests/test_glm_beta_gpu.py's inputs and bound quantities.  What the float32 formulas reach is printed (measured:
    ell 4e-8, T 5e-8, G 3e-7): the margin left for the device's reduction order and its library functions (a factor 20
    for ell and T at 2e-5, 100 for G at 1e-4)."""
    X, y, W, logprec, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S)
    r_ell, r_T, r_G = _f32_ratios(X, y, W, logprec, o, v)
    print("B=%d D=%d S=%d: ell err/bound quantity %.3g, T %.3g, G err/max %.3g" % (B, D, S, r_ell, r_T, r_G))
    assert r_ell <= 1e-6 and r_T <= 1e-6 and r_G <= 1e-6
    on = v > 0
    assert y[on].min() == np.float32(1e-6) and y[on].max() == np.float32(1.0 - 1e-6)
    assert logprec.min() == ref.TAU_LO and logprec.max() == ref.TAU_HI


@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
@pytest.mark.parametrize("flip", [1.0, -1.0])
def test_plain_float32_at_logits_of_eighty_is_finite_and_inside_the_bounds(D, B, flip):
    """make_extreme_inputs: logits of +-80 (flip = 1) and +-70 (flip = -1), tau in {-2, 0, 5}, y in {1e-6, 1/4, 1/2,
    1 - 1e-6}.  m phi goes down to e^{-82} = 2.4e-36 and psi(m phi) up to 4e35: every term is finite (measured: ell 6e-8,
    T 1e-7 of the bound quantities, G 2e-7 of its maximum)."""
    X, y, W, logprec, o, v = ref.make_extreme_inputs(D, B, flip)
    L = obs.logits(X, W, o)
    assert set(np.unique(np.abs(L[:, 0]))) == ({80.0} if flip > 0 else {70.0})
    assert (L[:, 0] > 0).any() and (L[:, 0] < 0).any() and set(logprec) == {-2.0, 0.0, 5.0}
    r_ell, r_T, r_G = _f32_ratios(X, y, W, logprec, o, v)
    print("D=%d flip=%g: ell err/bound quantity %.3g, T %.3g, G err/max %.3g" % (D, flip, r_ell, r_T, r_G))
    assert r_ell <= 1e-6 and r_T <= 1e-6 and r_G <= 1e-6


def test_float32_lgamma_and_psi_for_any_positive_argument():
    """The shifted product and three asymptotic terms from 1e-36 to 200: absolute errors within 1e-6 of the Stirling
    size plus |log min(x, 1)| (lnGamma) and of |psi(x)| + 3 (psi; the shifted asymptotic value is about log 8 = 2.1)."""
    x = np.concatenate([np.logspace(-36, 0, 400), np.linspace(1.0, 16.0, 601), np.linspace(16.0, 200.0, 300),
                        [1.0, 2.0, 7.9999995, 8.0, 8.000001]]).astype(np.float32)
    lg, ps = ref.lgamma_psi_f32(x)
    x64 = x.astype(np.float64)
    assert np.isfinite(lg).all() and np.isfinite(ps).all()
    e_lg = np.abs(lg - gammaln(x64)) / (ref.stirling_size(x64) + np.abs(np.log(np.minimum(x64, 1.0))))
    e_ps = np.abs(ps - digamma(x64)) / (np.abs(digamma(x64)) + 3.0)
    print("lnGamma %.3g, psi %.3g" % (e_lg.max(), e_ps.max()))
    assert e_lg.max() <= 1e-6 and e_ps.max() <= 1e-6


def test_predictive_reference_against_scipy():
    B, D, S = 120, 8, 16
    X, y, W, logprec, o, _ = ref.make_inputs(B, D, S, 4)
    out = ref.predict(X, W, logprec, y, o)
    L = obs.logits(X, W, o)
    phi = np.exp(logprec.astype(np.float64))[None, :]
    a, b = expit(L) * phi, expit(-L) * phi
    m, v = beta_dist.stats(a, b, moments="mv")
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-10)
    npt.assert_allclose(out["var"], v.mean(axis=1) + m.var(axis=1), rtol=1e-9)       # law of total variance
    lp = beta_dist.logpdf(y.astype(np.float64)[:, None], a, b)
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    bnd = ref.predict_bounds(X, W, logprec, y, o)
    assert all((bnd[k] > 0).all() for k in ("mean", "var", "lpd")) and bnd["lpd_sum"] > 0


def test_driver_argument_errors_need_no_device():
    from bayesic_amd.svi import BetaReparamSVI
    X = np.zeros((5, 4), np.float32)
    y = np.linspace(0.1, 0.9, 5)
    for wrong in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf, 0.99999999, 1e-50):
        bad = y.copy()
        bad[2] = wrong
        assert wrong != 0.99999999 or (wrong < 1.0 and np.float32(wrong) == 1.0)      # inside (0, 1) until it is rounded
        with pytest.raises(ValueError, match=r"strictly inside \(0, 1\) after rounding to float32"):
            BetaReparamSVI(X, bad)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the Beta model takes offset="):
        BetaReparamSVI(X, y, exposure=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="a0 and b0"):
        BetaReparamSVI(X, y, a0=0.0)
    with pytest.raises(ValueError, match="a0 and b0"):
        BetaReparamSVI(X, y, b0=-1.0)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        BetaReparamSVI(X, y, prior_precision=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        BetaReparamSVI(X, y, n_samples=65)
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        BetaReparamSVI(X, y, lam0=np.zeros(8))
    with pytest.raises(ValueError, match="covariance"):
        BetaReparamSVI(X, y, covariance="banded")


def test_set_batch_refuses_a_bad_response_before_anything_else():
    """set_batch checks y first; on a model that was never given a device that is all that runs."""
    import torch
    from bayesic_amd.svi import BetaReparamSVI
    m = BetaReparamSVI.__new__(BetaReparamSVI)
    X = torch.zeros((5, 4))
    for wrong in (0.0, 1.0, -2.0, float("nan"), float("inf")):
        y = torch.linspace(0.1, 0.9, 5)
        y[3] = wrong
        with pytest.raises(ValueError, match=r"strictly inside \(0, 1\) after rounding to float32"):
            m.set_batch(X, y)
    y64 = torch.linspace(0.1, 0.9, 5, dtype=torch.float64)
    y64[1] = 0.99999999
    with pytest.raises(ValueError, match=r"strictly inside \(0, 1\) after rounding to float32"):
        m.set_batch(X, y64)


def test_predict_routing_knows_the_family_and_leaves_the_pinned_tables_alone():
    from bayesic_amd import _ffi
    from bayesic_amd.svi import BetaReparamSVI, predict as mod
    m = BetaReparamSVI.__new__(BetaReparamSVI)
    assert mod.family_of(m) == "beta" and not mod.grouped(m)
    assert BetaReparamSVI.has_exposure is False and BetaReparamSVI.mean_key == "precision_mean"
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.SCALAR_FAMILIES == {"negbin": 0, "gamma": 1, "weibull": 2}
    assert mod.LOGIT_SCALAR_PASSES == {"beta": "bsc_beta_predict_pass"}
    for name, twin in (("bsc_glm_beta_data_pass", "bsc_glm_gamma_data_pass"), ("bsc_glm_beta_update", "bsc_glm_gamma_update"),
                       ("bsc_beta_predict_pass", "bsc_gamma_predict_pass")):
        assert _ffi.SIGNATURES[name] == _ffi.SIGNATURES[twin]
    # refusals that need no device: they are raised before the batch is touched
    X = np.zeros((3, 4), np.float32)
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not beta"):
        mod.predict(m, X, upper=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, groups=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the beta model takes offset="):
        mod.predict(m, X, exposure=np.ones(3, np.float32))
    m.has_offset = True
    with pytest.raises(ValueError, match="fitted with an offset"):
        mod.predict(m, X)


def test_reference_stepper_recovers_the_precision_on_the_recovery_data():
    """tests/test_glm_beta_gpu.py's recovery run in the float64 reference alone: 3 000 rows simulated at phi = 20, D = 8,
    300 full-batch updates (S = 8, lr = 0.05) under the default priors.  precision_mean lands at 19.89 (0.5 % below 20)
    and the weights within 0.06 of the truth: the 15 % of the GPU test holds for the reference on this seed with a
    factor 3 to spare (asserted at 5 %)."""
    R = ref.RECOVERY
    X, y, w_true = ref.recovery_data(R["seed"])
    X, y = X[:R["rows"]], y[:R["rows"]]
    B, D = X.shape
    assert B == 3000
    lam = ref.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, R["steps"] + 1):
        lam, m1, m2, elbo, _ = ref.step(lam, m1, m2, t, X, y, R["S"], R["driver_seed"], float(B), R["lr"], prec=1.0,
                                        a0=1.0, b0=0.1)
    phi_mean = math.exp(lam[D] + 0.5 * math.exp(2.0 * lam[2 * D + 1]))
    print("precision_mean %.4f, w err %.3g, ELBO %.6g" % (phi_mean, np.abs(lam[:D] - w_true).max(), elbo))
    assert np.isfinite(elbo)
    assert abs(phi_mean - 20.0) <= 0.15 * 20.0
    assert abs(phi_mean - 20.0) <= 0.05 * 20.0          # the margin the device run leans on
    assert np.abs(lam[:D] - w_true).max() < 0.1
