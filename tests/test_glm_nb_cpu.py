"""The float64 reference of the negative-binomial route (tests/_glm_nb_ref.py) checked against itself, scipy and the
Poisson reference, and what a float32 pass can reach against the device bounds; no device needed.

 * ell, G and T against central differences of the reference's own ell in w and tau;
 * the per-row log-pmf against scipy.stats.nbinom.logpmf(y, phi, phi / (phi + mu));
 * the Poisson limit at tau = 12 against tests/_glm_obs_ref.data_pass("poisson", ...), to the order y^2 / phi;
 * the finish against central differences of the ELBO in lam;
 * the predictive against nbinom's mean, variance and logpmf;
 * data_pass_f32 (naive float32, row after row) inside the device bounds of tests/test_glm_nb_gpu.py on its inputs;
 * the driver's argument errors that are raised before a device is asked for."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy.stats import nbinom

import _glm_nb_ref as ref
import _glm_obs_ref as obs


def _small(B, D, S, seed):
    """Inputs on a grid of 2^-12 so that w +- 2^-10 and tau +- 2^-10 are exact float32 values."""
    X, y, W, logphi, o, v = ref.make_inputs(B, D, S, seed)
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)
    return X, y, q(W), q(logphi), o, v


def test_G_and_T_are_the_derivatives_of_ell():
    B, D, S = 60, 4, 3
    X, y, W, logphi, o, v = _small(B, D, S, 1)
    ell, G, T = ref.data_pass(X, y, W, logphi, o, v)
    h = 2.0 ** -10
    for s in range(S):
        for d in range(D):
            Wp, Wm = W.copy(), W.copy()
            Wp[s, d] += h
            Wm[s, d] -= h
            fd = (ref.data_pass(X, y, Wp, logphi, o, v)[0][s] - ref.data_pass(X, y, Wm, logphi, o, v)[0][s]) / (2 * h)
            npt.assert_allclose(G[s, d], fd, rtol=1e-4, atol=1e-4 * np.abs(G).max())
        tp, tm = logphi.copy(), logphi.copy()
        tp[s] += h
        tm[s] -= h
        fd = (ref.data_pass(X, y, W, tp, o, v)[0][s] - ref.data_pass(X, y, W, tm, o, v)[0][s]) / (2 * h)
        npt.assert_allclose(T[s], fd, rtol=1e-4, atol=1e-4 * np.abs(T).max())
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_row_logpmf_is_scipys_negative_binomial():
    X, y, W, logphi, o, _ = ref.make_inputs(200, 8, 6, 2)
    L = obs.logits(X, W, o)
    phi = np.exp(logphi.astype(np.float64))[None, :]
    mu = np.exp(L)
    want = nbinom.logpmf(y.astype(np.float64)[:, None], phi, phi / (phi + mu))
    npt.assert_allclose(ref.row_logpmf(L, y, logphi), want, rtol=1e-10, atol=1e-9)
    # and ell is its sum with the constant -lnGamma(y + 1) left out
    from scipy.special import gammaln
    ell, _, _ = ref.data_pass(X, y, W, logphi, o, None)
    npt.assert_allclose(ell, (want + gammaln(y.astype(np.float64) + 1.0)[:, None]).sum(axis=0), rtol=1e-10)


def test_poisson_limit_at_large_dispersion():
    """tau = 12: ell - ell_Poisson = sum_n v_n ((y - mu)^2 - y) / (2 phi) + O(phi^-2), r - r_Poisson =
    -mu (y - mu) / (phi + mu), and T -> 0 at the same order.  Bounds: twice the leading terms."""
    B, D, S = 150, 8, 4
    rs = np.random.RandomState(3)
    X, _, W, _, o, v = ref.make_inputs(B, D, S, 3)
    y = rs.poisson(2.0, size=B).astype(np.float32)
    logphi = np.full(S, 12.0, np.float32)
    phi = math.exp(12.0)
    ell, G, T = ref.data_pass(X, y, W, logphi, o, v)
    ell_p, G_p = obs.data_pass("poisson", X, y, W, o, v)
    mu = np.exp(obs.logits(X, W, o))
    y64, v64 = y.astype(np.float64)[:, None], v.astype(np.float64)[:, None]
    lead = (v64 * ((y64 - mu) ** 2 + y64 + 1.0)).sum(axis=0) / phi
    assert (np.abs(ell - ell_p) <= lead).all()
    assert (np.abs(ell - ell_p) >= 1e-3 * lead).all()          # the limit is approached, not hit by construction
    g_lead = 2.0 * (v64 * mu * np.abs(y64 - mu)).T @ np.abs(X.astype(np.float64)) / phi
    assert (np.abs(G - G_p) <= g_lead + 1e-12).all()
    assert (np.abs(T) <= 2.0 * lead).all()


def test_reference_gradient_is_the_derivative_of_its_elbo():
    """Central differences of elbo_fixed_draws in every coordinate of lam (tests/test_glm_group_cpu.py's form)."""
    B, D, S = 80, 4, 5
    X, y, _, _, o, v = ref.make_inputs(B, D, S, 1)
    y = np.minimum(y, 40.0).astype(np.float32)
    P = D + 1
    rs = np.random.RandomState(2)
    lam = np.concatenate([0.3 * rs.standard_normal(P), math.log(0.2) + 0.1 * rs.standard_normal(P)])
    eps = ref.noise(D, S, 7, 0)
    scale, prec, a0, b0 = 3.0, 1.7, 1.5, 0.8
    W, logphi = ref.draw(lam, eps)
    ell, G, T = ref.data_pass(X, y, W, logphi, o, v)
    _, grad = ref.elbo_and_grad(lam, eps, W, logphi, ell, G, T, scale, prec, a0, b0)
    h = 1e-5
    fd = np.zeros_like(lam)
    for i in range(2 * P):
        e = np.zeros_like(lam)
        e[i] = h
        fd[i] = (ref.elbo_fixed_draws(lam + e, eps, X, y, scale, prec, a0, b0, o, v)
                 - ref.elbo_fixed_draws(lam - e, eps, X, y, scale, prec, a0, b0, o, v)) / (2 * h)
    assert np.abs(grad - fd).max() <= 1e-4 * np.abs(fd).max(), np.abs(grad - fd).max() / np.abs(fd).max()
    for lo, hi in ((0, D), (D, P)):                              # w and tau each carry a gradient worth checking
        assert np.abs(fd[lo:hi]).max() > 1e-2 and np.abs(fd[P + lo:P + hi]).max() > 1e-3
    # the ELBO value itself, from the same draws
    elbo, _ = ref.elbo_and_grad(lam, eps, W, logphi, ell, G, T, scale, prec, a0, b0)
    npt.assert_allclose(elbo, ref.elbo_fixed_draws(lam, eps, X, y, scale, prec, a0, b0, o, v), rtol=1e-6)


def test_predictive_reference_against_scipy():
    B, D, S = 120, 8, 16
    X, y, W, logphi, o, _ = ref.make_inputs(B, D, S, 4)
    out = ref.predict(X, W, logphi, y, o)
    L = obs.logits(X, W, o)
    phi = np.exp(logphi.astype(np.float64))[None, :]
    mu = np.exp(L)
    p = phi / (phi + mu)
    m, v = nbinom.stats(phi, p, moments="mv")
    npt.assert_allclose(out["mean"], m.mean(axis=1), rtol=1e-10)
    npt.assert_allclose(out["var"], v.mean(axis=1) + m.var(axis=1), rtol=1e-9)       # law of total variance
    lp = nbinom.logpmf(y.astype(np.float64)[:, None], phi, p)
    npt.assert_allclose(out["lpd"], np.log(np.exp(lp).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    b = ref.predict_bounds(X, W, logphi, y, o)
    assert all((b[k] > 0).all() for k in ("mean", "var", "lpd")) and b["lpd_sum"] > 0


@pytest.mark.parametrize("B,D,S", [(37, 64, 11), (165, 252, 11), (325, 256, 11), (1003, 256, 8)])
def test_naive_float32_stays_inside_the_device_bounds(B, D, S):
    """tests/test_glm_nb_gpu.py's inputs and bounds: ell and T within 2e-5 of their bound quantities, G within rtol 1e-4
    and atol 1e-4 max|G|.  What the float32 formulas reach is printed: the margin left for the device's reduction order
    and fast intrinsics."""
    X, y, W, logphi, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S)
    ell, G, T = ref.data_pass_f32(X, y, W, logphi, o, v)
    ell_r, G_r, T_r = ref.data_pass(X, y, W, logphi, o, v)
    b_ell, b_T = ref.bounds(X, y, W, logphi, o, v)
    r_ell = (np.abs(ell - ell_r) / b_ell).max()
    r_T = (np.abs(T - T_r) / b_T).max()
    r_G = np.abs(G - G_r).max() / np.abs(G_r).max()
    print("B=%d D=%d S=%d: ell err/bound quantity %.3g, T %.3g, G err/max %.3g" % (B, D, S, r_ell, r_T, r_G))
    assert r_ell <= 2e-5 and r_T <= 2e-5
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    assert y.max() >= 100 and (y == 0).sum() > B // 8


def test_driver_argument_errors_need_no_device():
    from bayesic_amd.svi import NegBinReparamSVI
    X = np.zeros((5, 4), np.float32)
    y = np.arange(5, dtype=np.float32)
    bad = y.copy()
    bad[2] = -1.0
    with pytest.raises(ValueError, match="y must be finite and >= 0"):
        NegBinReparamSVI(X, bad)
    bad[2] = np.nan
    with pytest.raises(ValueError, match="y must be finite and >= 0"):
        NegBinReparamSVI(X, bad)
    with pytest.raises(ValueError, match="exposure and offset are mutually exclusive"):
        NegBinReparamSVI(X, y, offset=np.zeros(5, np.float32), exposure=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="a0 and b0"):
        NegBinReparamSVI(X, y, a0=0.0)
    with pytest.raises(ValueError, match="a0 and b0"):
        NegBinReparamSVI(X, y, b0=-1.0)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        NegBinReparamSVI(X, y, prior_precision=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        NegBinReparamSVI(X, y, n_samples=65)
