"""The float64 reference of the Gamma route (tests/_glm_gamma_ref.py) checked against scipy and itself, what a float32
pass can reach against the device bounds, the driver's refusals, and the update rule against maximum likelihood; no
device needed.

 * the per-row log density against scipy.stats.gamma.logpdf(y, alpha, scale=mu / alpha), rtol 1e-9;
 * G and T against central differences of the reference's own ell in w and tau;
 * data_pass_f32 (plain float32, row after row) below 1e-6 of b_ell, b_T and max|G| on make_inputs: the headroom the
   tolerances of tests/test_glm_gamma_gpu.py (2e-5 and 1e-4) lean on;
 * the predictive against scipy's mean, variance and logpdf;
 * the driver's argument errors that are raised before a device is asked for;
 * the reference stepper, from a fixed seed, against the maximum-likelihood (w, alpha) of simulated data."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.optimize import minimize
from scipy.stats import gamma as gamma_dist

import _glm_gamma_ref as ref
import _glm_obs_ref as obs


def _small(B, D, S, seed):
    """Inputs on a grid of 2^-12 so that w +- 2^-10 and tau +- 2^-10 are exact float32 values."""
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed)
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)
    return X, y, q(W), q(logshape), o, v


def test_row_logpdf_is_scipys_gamma():
    X, y, W, logshape, o, _ = ref.make_inputs(200, 8, 6, 2)
    L = obs.logits(X, W, o)
    alpha = np.exp(logshape.astype(np.float64))[None, :]
    mu = np.exp(L)
    want = gamma_dist.logpdf(y.astype(np.float64)[:, None], alpha, scale=mu / alpha)
    npt.assert_allclose(ref.row_logpdf(L, y, logshape), want, rtol=1e-9)
    assert y.max() / y.min() > 1e6 and logshape.min() < 0.0 < 2.0 < logshape.max()
    # and ell is its sum: nothing is left out
    ell, _, _ = ref.data_pass(X, y, W, logshape, o, None)
    npt.assert_allclose(ell, want.sum(axis=0), rtol=1e-9)


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 60, 4, 3
    X, y, W, logshape, o, v = _small(B, D, S, 1)
    ell, G, T = ref.data_pass(X, y, W, logshape, o, v)
    h = 2.0 ** -10
    for s in range(S):
        for d in range(D):
            Wp, Wm = W.copy(), W.copy()
            Wp[s, d] += h
            Wm[s, d] -= h
            fd = (ref.data_pass(X, y, Wp, logshape, o, v)[0][s] - ref.data_pass(X, y, Wm, logshape, o, v)[0][s]) / (2 * h)
            npt.assert_allclose(G[s, d], fd, rtol=1e-4, atol=1e-4 * np.abs(G).max())
        tp, tm = logshape.copy(), logshape.copy()
        tp[s] += h
        tm[s] -= h
        fd = (ref.data_pass(X, y, W, tp, o, v)[0][s] - ref.data_pass(X, y, W, tm, o, v)[0][s]) / (2 * h)
        npt.assert_allclose(T[s], fd, rtol=1e-4, atol=1e-4 * np.abs(T).max())
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, logshape, o, v = ref.make_inputs(40, 8, 4, 3)
    v[37:] = 0.0
    y[37:] = [1.0e30, 0.0, -5.0]
    o[37:] = [200.0, -1.0e30, 1.0e30]
    a = ref.data_pass(X, y, W, logshape, o, v)
    b = ref.data_pass(X[:37], y[:37], W, logshape, o[:37], v[:37])
    for p, q in zip(a, b):
        assert np.isfinite(p).all()
        npt.assert_array_equal(p, q)


@pytest.mark.parametrize("B,D,S", [(37, 64, 11), (165, 252, 11), (325, 256, 11), (1003, 256, 8)])
def test_plain_float32_stays_below_1e_6_of_the_bound_quantities(B, D, S):
    """tests/test_glm_gamma_gpu.py's inputs and bound quantities.  What the float32 formulas reach is printed: the
    margin left for the device's reduction order (a factor 20 for ell and T at 2e-5, 100 for G at 1e-4).  The sums are
    float32 over 64 rows and float64 above, as the pass's are (tests/_glm_gamma_ref.data_pass_f32 says why)."""
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S)
    ell, G, T = ref.data_pass_f32(X, y, W, logshape, o, v)
    ell_r, G_r, T_r = ref.data_pass(X, y, W, logshape, o, v)
    b_ell, b_T = ref.bounds(X, y, W, logshape, o, v)
    r_ell = (np.abs(ell - ell_r) / b_ell).max()
    r_T = (np.abs(T - T_r) / b_T).max()
    r_G = np.abs(G - G_r).max() / np.abs(G_r).max()
    print("B=%d D=%d S=%d: ell err/bound quantity %.3g, T %.3g, G err/max %.3g" % (B, D, S, r_ell, r_T, r_G))
    assert r_ell <= 1e-6 and r_T <= 1e-6 and r_G <= 1e-6
    on = v > 0
    assert y[on].max() / y[on].min() > 1e5 and -2.5 <= logshape.min() and logshape.max() <= 5.0


def test_predictive_reference_against_scipy():
    B, D, S = 120, 8, 16
    X, y, W, logshape, o, _ = ref.make_inputs(B, D, S, 4)
    out = ref.predict(X, W, logshape, y, o)
    L = obs.logits(X, W, o)
    alpha = np.exp(logshape.astype(np.float64))[None, :]
    mu = np.exp(L)
    m, v = gamma_dist.stats(alpha, scale=mu / alpha, moments="mv")
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-10)
    npt.assert_allclose(out["var"], v.mean(axis=1) + m.var(axis=1), rtol=1e-9)       # law of total variance
    lp = gamma_dist.logpdf(y.astype(np.float64)[:, None], alpha, scale=mu / alpha)
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    b = ref.predict_bounds(X, W, logshape, y, o)
    assert all((b[k] > 0).all() for k in ("mean", "var", "lpd")) and b["lpd_sum"] > 0


def test_driver_argument_errors_need_no_device():
    from bayesic_amd.svi import GammaReparamSVI
    X = np.zeros((5, 4), np.float32)
    y = np.arange(1, 6, dtype=np.float32)
    for wrong in (0.0, -1.0, np.nan, np.inf):
        bad = y.copy()
        bad[2] = wrong
        with pytest.raises(ValueError, match="y must be finite and > 0"):
            GammaReparamSVI(X, bad)
    with pytest.raises(ValueError, match="exposure and offset are mutually exclusive"):
        GammaReparamSVI(X, y, offset=np.zeros(5, np.float32), exposure=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="a0 and b0"):
        GammaReparamSVI(X, y, a0=0.0)
    with pytest.raises(ValueError, match="a0 and b0"):
        GammaReparamSVI(X, y, b0=-1.0)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        GammaReparamSVI(X, y, prior_precision=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        GammaReparamSVI(X, y, n_samples=65)
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        GammaReparamSVI(X, y, lam0=np.zeros(8))


def test_set_batch_refuses_a_bad_response_before_anything_else():
    """set_batch checks y first; on a model that was never given a device that is all that runs."""
    import torch
    from bayesic_amd.svi import GammaReparamSVI
    m = GammaReparamSVI.__new__(GammaReparamSVI)
    X = torch.zeros((5, 4))
    for wrong in (0.0, -2.0, float("nan"), float("inf")):
        y = torch.arange(1, 6, dtype=torch.float32)
        y[3] = wrong
        with pytest.raises(ValueError, match="y must be finite and > 0"):
            m.set_batch(X, y)


def test_reference_stepper_reaches_the_maximum_likelihood_fit():
    """600 rows simulated at alpha = 3 with an offset; 400 full-batch updates of the reference stepper (S = 8, lr = 0.05,
    then 200 at lr = 0.01 to settle Adam's wander) under wide priors.  The maximum-likelihood (w, tau) comes from
    scipy.optimize on the negative sum of scipy's own logpdf.  The stepper's means sit within three of its own posterior
    standard deviations of it: the update rule climbs the right function."""
    rs = np.random.RandomState(21)
    B, D, S, seed = 600, 4, 8, 99
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    X[:, 0] = 1.0
    o = (0.5 * rs.standard_normal(B)).astype(np.float32)
    w_true = np.array([0.8, -0.6, 0.4, 0.3])
    mu = np.exp(X.astype(np.float64) @ w_true + o)
    y = rs.gamma(3.0, mu / 3.0).astype(np.float32)
    X64, y64, o64 = X.astype(np.float64), y.astype(np.float64), o.astype(np.float64)

    def nll(p):
        a = math.exp(p[D])
        return -gamma_dist.logpdf(y64, a, scale=np.exp(X64 @ p[:D] + o64) / a).sum()

    ml = minimize(nll, np.zeros(D + 1), method="BFGS", options=dict(gtol=1e-8))
    assert ml.success or ml.fun < nll(np.zeros(D + 1))
    assert abs(math.exp(ml.x[D]) - 3.0) < 0.6                    # the simulation itself is sane

    lam = ref.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 601):
        lam, m1, m2, elbo, _ = ref.step(lam, m1, m2, t, X, y, S, seed, float(B), 0.05 if t <= 400 else 0.01,
                                        prec=1e-2, a0=1.0, b0=0.1, offset=o)
    P = D + 1
    z = (lam[:P] - ml.x) / np.exp(lam[P:])
    print("ML", ml.x, "m", lam[:P], "sd", np.exp(lam[P:]), "z", z)
    assert np.isfinite(elbo)
    assert np.abs(z).max() <= 3.0, z
    # and the posterior is not vacuously wide: every standard deviation is below a tenth
    assert np.exp(lam[P:]).max() < 0.1
