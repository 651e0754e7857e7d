"""The float64 reference of the posterior predictive (tests/_predict_ref.py) against scipy and against closed forms,
the draw layout of the three guides, and ReparamVI.predict's refusal off the fused routes.  No GPU."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy import special, stats

import _fullrank_ref as fr
import _predict_ref as ref
from oracle import philox


def _case(family, B=40, D=12, S=9, seed=0):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.8 * rs.standard_normal((S, D))).astype(np.float32)
    logvar = rs.uniform(-2.0, 1.0, S).astype(np.float32) if family == "gaussian" else None
    y = {"gaussian": rs.standard_normal(B), "logistic": (rs.uniform(size=B) < 0.5) * 1.0,
         "poisson": rs.poisson(1.5, B) * 1.0}[family].astype(np.float32)
    return X, W, logvar, y


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_log_density_matches_scipy(family):
    X, W, logvar, y = _case(family)
    L = ref.logits(X, W)
    got = ref.log_p(family, L, y, logvar)
    y64 = y.astype(np.float64)[:, None]
    if family == "gaussian":
        want = stats.norm.logpdf(y64, loc=L, scale=np.exp(0.5 * logvar.astype(np.float64))[None, :])
    elif family == "logistic":
        want = stats.bernoulli.logpmf(y64, special.expit(L))
    else:
        want = stats.poisson.logpmf(y64, np.exp(L))
    npt.assert_allclose(got, want, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_lpd_and_variance_match_scipy_and_numpy(family):
    X, W, logvar, y = _case(family, seed=3)
    out = ref.predict(family, X, W, logvar, y)
    L = ref.logits(X, W)
    S = W.shape[0]
    npt.assert_allclose(out["lpd"], special.logsumexp(ref.log_p(family, L, y, logvar), axis=1) - math.log(S), rtol=1e-13)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-15)
    mu, v = ref.moments(family, L, logvar)
    npt.assert_allclose(out["mean"], np.mean(mu, axis=1), rtol=1e-15)
    npt.assert_allclose(out["var"], v.mean(axis=1) + np.var(mu, axis=1), rtol=1e-12)
    # log-mean-exp, not mean-log: Jensen's gap is strictly positive as soon as the draws disagree
    assert (out["lpd"] > ref.log_p(family, L, y, logvar).mean(axis=1)).all()


def test_gaussian_predictive_of_a_full_covariance_guide_is_the_closed_form():
    """xi spread 0 (its row of L is ~0), so sigma^2 = e^{mu_xi} and the predictive of row x is
    N(x . mu_w, sigma^2 + x^T Sigma x).  S = 4096 draws of the reference's own layout; five Monte Carlo standard
    errors: se(mean) = sqrt(x^T Sigma x / S), se(var) = x^T Sigma x sqrt(2 / (S - 1)) for a Gaussian sample variance."""
    D, S, seed = 6, 4096, 17
    P = D + 1
    rs = np.random.RandomState(5)
    L = np.tril(0.3 * rs.standard_normal((P, P)))
    L[np.arange(P), np.arange(P)] = np.exp(rs.uniform(-1.5, -0.5, P))
    L[D, :] = 0.0
    L[D, D] = 1e-12
    mu = np.concatenate([rs.standard_normal(D), [math.log(0.7)]])
    lam = fr.pack(mu, L)
    W, logvar = ref.posterior_draws("full", lam, D, S, seed)
    npt.assert_allclose(logvar, math.log(0.7), rtol=1e-6)
    X = rs.standard_normal((8, D)).astype(np.float32)
    out = ref.predict("gaussian", X, W, logvar)
    X64 = X.astype(np.float64)
    Sigma = (L @ L.T)[:D, :D]
    q = np.einsum("nd,de,ne->n", X64, Sigma, X64)
    z_mean = np.abs(out["mean"] - X64 @ mu[:D]) / np.sqrt(q / S)
    z_var = np.abs(out["var"] - (0.7 + q)) / (q * math.sqrt(2.0 / (S - 1)))
    print("z(mean) max %.2f, z(var) max %.2f" % (z_mean.max(), z_var.max()))
    assert (z_mean < 5.0).all() and (z_var < 5.0).all()


def test_draw_layout_of_the_three_guides():
    D, S, seed = 5, 7, 99
    rs = np.random.RandomState(1)
    eps_w = philox.normal_draws(seed, S, D, stream=ref.STREAM, step=0)
    eps_z = philox.normal_draws(seed, S, D + 1, stream=ref.STREAM, step=0)
    for other in (0, 1):   # the training streams give other numbers
        assert np.abs(eps_w - philox.normal_draws(seed, S, D, stream=other, step=0)).min() > 0
    # glm: lam = [m | rho]
    lam = np.concatenate([rs.standard_normal(D), rs.uniform(-2, 0, D)])
    W, lv = ref.posterior_draws("glm", lam, D, S, seed)
    assert lv is None and W.dtype == np.float32 and W.shape == (S, D)
    for s in range(S):
        for d in range(D):
            assert W[s, d] == np.float32(lam[d] + math.exp(lam[D + d]) * eps_w[s, d])
    # diag: lam = [m | rho | a | b]; xi from column D of the same block
    lam = np.concatenate([rs.standard_normal(D), rs.uniform(-2, 0, D), [0.3, -1.0]])
    W, lv = ref.posterior_draws("diag", lam, D, S, seed)
    npt.assert_array_equal(W, (lam[:D] + np.exp(lam[D:2 * D]) * eps_z[:, :D]).astype(np.float32))
    npt.assert_array_equal(lv, (0.3 + math.exp(-1.0) * eps_z[:, D]).astype(np.float32))
    # full with a diagonal L is the mean-field draw; an off-diagonal entry L[i, j] moves z_i by L[i, j] eps_j
    full = fr.from_mean_field(lam, D)
    W2, lv2 = ref.posterior_draws("full", full, D, S, seed)
    npt.assert_allclose(W2, W, rtol=1e-6)
    npt.assert_allclose(lv2, lv, rtol=1e-6)
    mu, L = fr.unpack(full, D + 1)
    L[D, 1] = 0.5           # xi picks up eps_1
    L[3, 0] = -0.25         # w_3 picks up eps_0
    W3, lv3 = ref.posterior_draws("full", fr.pack(mu, L), D, S, seed)
    npt.assert_allclose(lv3 - lv2, 0.5 * eps_z[:, 1], atol=1e-6)
    npt.assert_allclose(W3[:, 3] - W2[:, 3], -0.25 * eps_z[:, 0], atol=1e-6)
    npt.assert_array_equal(np.delete(W3, 3, axis=1), np.delete(W2, 3, axis=1))


def test_the_public_module_is_exported_and_validates_without_a_device():
    from bayesic_amd import svi
    from bayesic_amd.svi import predict as mod
    assert svi.posterior_draws is mod.posterior_draws and svi.heldout_lpd is mod.heldout_lpd
    assert mod.PREDICT_STREAM == ref.STREAM and mod.FAMILIES == ref.CODE

    class Fake:
        family = (0.0, 1.0, 1.0, 1.0, 1.0)
    with pytest.raises(NotImplementedError, match="precision"):
        mod.family_of(Fake())
    with pytest.raises(ValueError, match="at most 64"):
        mod.posterior_draws(Fake(), n_samples=65)


def test_reparam_vi_refuses_to_predict_on_a_general_route():
    from oracle.einsum_eval import NumpyBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint
    rs = np.random.RandomState(0)
    X = rs.standard_normal((50, 4))
    y = (rs.uniform(size=50) < 0.5) * 1.0
    lj, v = logistic_regression_log_joint(1.0, 1.0)
    eng = ReparamVI(lj, [(v["W"], 4)], dict(X=X, y=y), n_samples=4, seed=1, backend=NumpyBackend(np.float64))
    assert eng.route == "general"
    with pytest.raises(NotImplementedError, match="route 'general'"):
        eng.predict(X)
