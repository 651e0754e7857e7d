"""The GLM path on the CPU: the float64 reference (tests/_glm_ref.py) against finite differences and scipy's
densities, and ``recognise.glm_linear`` -- which symbolic log-joints are read as a Bernoulli-logit or Poisson-log
regression with an isotropic Gaussian prior, and which are left alone."""
import math

import numpy as np
import numpy.testing as npt
import pytest

from bayesic_amd import algebra as A
from bayesic_amd.inference import recognise as R
from bayesic_amd.inference.models import (linear_regression_log_joint, logistic_regression_log_joint,
                                          poisson_regression_log_joint)

import _glm_ref as ref

N, D, S = 1000, 16, 8
SHAPES = {"X": (N, D), "y": (N,)}
LINKS = ("logistic", "poisson")


def _data(link, n, d, seed=0):
    rng = np.random.RandomState(seed)
    X = (rng.standard_normal((n, d)) / math.sqrt(d)).astype(np.float32)
    w = rng.standard_normal(d)
    L = X.astype(np.float64) @ w
    if link == "logistic":
        y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-L))).astype(np.float32)
    else:
        y = rng.poisson(np.exp(L)).astype(np.float32)
    return X, y


@pytest.mark.parametrize("link", LINKS)
def test_reference_gradient_is_the_derivative_of_its_own_elbo(link):
    """Central finite differences of the ELBO estimate with the draws held fixed (all float64, draws not rounded)."""
    n, d, s, scale, tau = 200, 6, 5, 3.0, 0.7
    X, y = _data(link, n, d)
    rng = np.random.RandomState(1)
    lam = np.concatenate([0.3 * rng.standard_normal(d), np.log(0.2) + 0.1 * rng.standard_normal(d)])
    eps = ref.noise(d, s, 77, 3)
    W = lam[None, :d] + np.exp(lam[d:])[None, :] * eps          # float64 draws: the smooth function's own
    L = X.astype(np.float64) @ W.T
    Apart, dA = ref.log_partition(link, L)
    ell = (y.astype(np.float64)[:, None] * L - Apart).sum(axis=0)
    G = (y.astype(np.float64)[:, None] - dA).T @ X.astype(np.float64)
    elbo, grad = ref.glm_elbo_and_grad(lam, eps, W, ell, G, scale, tau)
    npt.assert_allclose(elbo, ref.elbo_fixed_draws(link, lam, eps, X, y, scale, tau), rtol=1e-13)
    h = 1e-5
    for i in range(2 * d):
        e = np.zeros(2 * d)
        e[i] = h
        fd = (ref.elbo_fixed_draws(link, lam + e, eps, X, y, scale, tau)
              - ref.elbo_fixed_draws(link, lam - e, eps, X, y, scale, tau)) / (2 * h)
        npt.assert_allclose(grad[i], fd, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("link", LINKS)
def test_reference_data_term_is_the_log_density(link):
    from scipy import stats
    from scipy.special import gammaln
    X, y = _data(link, 300, 8, seed=4)
    W = (0.5 * np.random.RandomState(5).standard_normal((3, 8))).astype(np.float32)
    ell, _ = ref.glm_data_pass(link, X, y, W)
    L = X.astype(np.float64) @ W.astype(np.float64).T
    for s in range(3):
        if link == "logistic":
            want = stats.bernoulli.logpmf(y.astype(int), 1.0 / (1.0 + np.exp(-L[:, s]))).sum()
            npt.assert_allclose(ell[s], want, rtol=1e-12)
        else:
            want = stats.poisson.logpmf(y.astype(int), np.exp(L[:, s])).sum()
            npt.assert_allclose(ell[s] - gammaln(y.astype(np.float64) + 1.0).sum(), want, rtol=1e-12)


def test_reference_step_moves_towards_the_data():
    X, y = _data("logistic", 500, 4, seed=2)
    lam = ref.init_lam(4)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    first = None
    for t in range(1, 60):
        lam, m1, m2, elbo, _ = ref.glm_step("logistic", lam, m1, m2, t, X, y, 8, 3, 500.0, 0.05)
        first = elbo if first is None else first
    assert elbo > first


def _written(link, writing, scale, tau):
    """The same model in several writings; every one must be recognised with the same (link, scale, tau)."""
    X, y, W = A.var("X", 2), A.var("y", 1), A.var("W", 2)
    l = A.dot(W, X.T)
    yb = A.dimshuffle(y, "x", 0)
    part = A.log(1.0 + A.exp(l)) if link == "logistic" else A.exp(l)
    prior = A.sum(W * W, axis=1) * (-0.5 * tau)
    if writing == "builder":                    # scale outside the sum, the prior's normaliser kept
        fn = logistic_regression_log_joint if link == "logistic" else poisson_regression_log_joint
        lj, v = fn(scale, tau)
        return lj, v["W"]
    if writing == "scale inside, constants dropped":
        return A.sum(yb * l * scale - part * scale, axis=1) + prior, W
    if writing == "two sums, a constant per row kept":
        return (A.sum(yb * l, axis=1) - A.sum(part, axis=1)) * scale + prior + A.shape(X, 0) * (-0.25) + 1.5, W
    raise ValueError(writing)


@pytest.mark.parametrize("writing", ["builder", "scale inside, constants dropped", "two sums, a constant per row kept"])
@pytest.mark.parametrize("link", LINKS)
def test_both_links_are_recognised_however_they_are_written(link, writing):
    scale, tau = 37.5, 2.5
    lj, W = _written(link, writing, scale, tau)
    why = []
    plan = R.glm_linear(lj, [(W, D)], SHAPES, S, why=why)
    assert plan is not None, why
    assert (plan.link, plan.X, plan.y, plan.W) == (link, "X", "y", "W")
    npt.assert_allclose([plan.scale, plan.tau], [scale, tau], rtol=1e-9)


def test_what_is_not_such_a_glm_is_declined_with_a_reason():
    X, y, W = A.var("X", 2), A.var("y", 1), A.var("W", 2)
    l = A.dot(W, X.T)
    yb = A.dimshuffle(y, "x", 0)
    bern = A.sum(yb * l - A.log(1.0 + A.exp(l)), axis=1)

    def declined(lj, latents, shapes=SHAPES):
        why = []
        assert R.glm_linear(lj, latents, shapes, S, why=why) is None
        assert why and why[-1]
        return why[-1]

    # the Gaussian model (config 2): two latent blocks
    lj, v = linear_regression_log_joint(3.0, 1.0, 1.0)
    assert "one latent block" in declined(lj, [(v["W"], D), (v["xi"], 1)])
    # ... and with a known noise variance: one block, but not this likelihood
    r = yb - l
    declined(A.sum(r * r, axis=1) * (-2.0) + A.sum(W * W, axis=1) * (-0.5), [(W, D)])
    # a hierarchical logistic model: group intercepts and their log precision on top of the weights
    Gm, Bv, Z = A.var("Gm", 2), A.var("B", 2), A.var("zeta", 2)
    lh = l + A.dot(Bv, Gm.T)
    z = A.sum(Z, axis=1)
    hier = A.sum(yb * lh - A.log(1.0 + A.exp(lh)), axis=1) + A.sum(W * W, axis=1) * (-0.5) \
        + A.sum(Bv * Bv, axis=1) * A.exp(z) * (-0.5) + z * 2.0 - A.exp(z)
    shapes = dict(SHAPES, Gm=(N, 5))
    assert "one latent block" in declined(hier, [(W, D), (Bv, 5), (Z, 1)], shapes)
    # a non-isotropic prior: precisions 1, 2, ..., D
    prec = A.constant(np.arange(1.0, D + 1.0)[None, :])
    declined(bern + A.sum(W * W * prec, axis=1) * (-0.5), [(W, D)])
    # no prior at all is no proper N(0, I / tau)
    assert "tau" in declined(bern * 2.0, [(W, D)])
    # a negative scale
    assert "positive" in declined(bern * (-2.0) + A.sum(W * W, axis=1) * (-0.5), [(W, D)])
    # a probit-like link is not one of the two
    declined(A.sum(yb * l - A.log(1.0 + A.exp(l * 1.7)), axis=1) + A.sum(W * W, axis=1) * (-0.5), [(W, D)])


def test_the_gaussian_model_keeps_its_own_recogniser():
    lj, v = linear_regression_log_joint(10.0, 2.5, 0.7)
    latents = [(v["W"], D), (v["xi"], 1)]
    plan = R.gaussian_linear(lj, latents, SHAPES, S)
    assert plan is not None and plan.family is not None
    assert R.glm_linear(lj, latents, SHAPES, S) is None
    # and the GLMs are none of gaussian_linear's business
    for fn in (logistic_regression_log_joint, poisson_regression_log_joint):
        lj, v = fn(4.0, 1.0)
        assert R.gaussian_linear(lj, [(v["W"], D)], SHAPES, S) is None
        assert R.glm_linear(lj, [(v["W"], D)], SHAPES, S) is not None


def test_driver_and_entry_points_are_declared():
    from bayesic_amd import _ffi
    from bayesic_amd.svi import GLMReparamSVI
    assert GLMReparamSVI.__init__.__defaults__[0] == "logistic"
    for name in ("bsc_glm_data_pass", "bsc_glm_update", "bsc_glm_pass_update"):
        assert name in _ffi.SIGNATURES
