"""CPU checks of the random-intercept routes of the families with a learned scalar: the float64 reference
(tests/_glm_scalar_group_ref.py) against numerical derivatives of itself, the simulated fit both GPU end-to-end tests
assert on, and the constructor refusals that need no device."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import _glm_scalar_group_ref as ref

FAMILIES = ref.FAMILIES


def _small(fam, seed=3, B=60, D=4, J=5, S=3):
    """A small batch whose draws lie on a dyadic grid, so that b +- h and tau +- h are float32 values: the reference
    rounds its operands to float32, and a step that is not representable would not be the step taken."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    W = (0.4 * rs.standard_normal((S, D))).astype(np.float32)
    Bm = (np.round(0.5 * rs.standard_normal((S, J)) * 256) / 256).astype(np.float32)
    logtau = (np.round(rs.uniform(-0.5, 1.0, S) * 256) / 256).astype(np.float32)
    o = (0.3 * rs.standard_normal(B)).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::5] = 0.0
    if fam == "negbin":
        y = rs.poisson(1.5, size=B).astype(np.float32)
    elif fam == "gamma":
        y = rs.gamma(2.0, 0.7, size=B).astype(np.float32)
    else:
        y = (rs.weibull(1.5, size=B) * np.where(rs.uniform(size=B) < 0.3, -1.0, 1.0)).astype(np.float32)
    return X, y, g, J, W, Bm, logtau, o, v


@pytest.mark.parametrize("fam", FAMILIES)
def test_H_and_T_are_the_derivatives_of_ell(fam):
    """Central differences with h = 2^-10 (exact in float32 on the grid of _small): the truncation error is h^2 / 6 of the
    third derivative, 1.6e-7 of it; the assertion allows 1e-5 of the T bound (the sum of the sizes of T's terms)."""
    X, y, g, J, W, Bm, logtau, o, v = _small(fam)
    h = 2.0 ** -10
    ell, G, H, T = ref.data_pass(fam, X, y, g, J, W, Bm, logtau, o, v)
    b_T = ref.bounds(fam, X, y, g, J, W, Bm, logtau, o, v)[1]
    for j in range(J):
        up, dn = Bm.copy(), Bm.copy()
        up[:, j] += np.float32(h)
        dn[:, j] -= np.float32(h)
        d = (ref.data_pass(fam, X, y, g, J, W, up, logtau, o, v)[0]
             - ref.data_pass(fam, X, y, g, J, W, dn, logtau, o, v)[0]) / (2 * h)
        assert (np.abs(d - H[:, j]) <= 1e-5 * b_T).all(), (fam, j, d, H[:, j])
    d = (ref.data_pass(fam, X, y, g, J, W, Bm, logtau + np.float32(h), o, v)[0]
         - ref.data_pass(fam, X, y, g, J, W, Bm, logtau - np.float32(h), o, v)[0]) / (2 * h)
    assert (np.abs(d - T) <= 1e-5 * b_T).all(), (fam, d, T)
    # H is the one-hot columns' share of the residuals: its rows add up to what an all-ones column would collect
    ones = np.ones((X.shape[0], 1), np.float32)
    G1 = ref.MOD[fam].data_pass(np.concatenate([ref.design(X, g, J), ones], axis=1), y,
                                np.concatenate([ref.draws(W, Bm), np.zeros((W.shape[0], 1), np.float32)], axis=1),
                                logtau, o, v)[1]
    npt.assert_allclose(H.sum(axis=1), G1[:, -1], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("fam", FAMILIES)
def test_loglik64_is_the_family_helpers_ell_at_float32_draws(fam):
    X, y, g, J, W, Bm, logtau, o, _ = _small(fam, seed=4)
    L = ref.grp.logits(X, g, W, Bm, o)
    ell = ref.data_pass(fam, X, y, g, J, W, Bm, logtau, o, None)[0]
    npt.assert_allclose(ref.loglik64(fam, L, y, logtau), ell, rtol=1e-12)


@pytest.mark.parametrize("fam", FAMILIES)
def test_restated_gradient_is_the_derivative_of_the_restated_elbo(fam):
    """At fixed draws, all float64.  The statistics are taken at the unrounded draws (float64 in, through the same
    formulas), so the two sides differ by the central difference's truncation alone."""
    X, y, g, J, _, _, _, o, _ = _small(fam, seed=6)
    D, S = X.shape[1], 3
    P = D + J + 2
    rs = np.random.RandomState(8)
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.2) + 0.1 * rs.standard_normal(P)])
    eps = ref.noise(D, J, S, 11, 0)
    scale, prec, a0, b0, ga0, gb0 = 3.0, 1.7, 1.5, 0.4, 1.2, 0.9
    z = lam[None, :P] + np.exp(lam[P:])[None, :] * eps
    w, b, zeta, tau = z[:, :D], z[:, D:D + J], z[:, P - 2], z[:, P - 1]
    # the statistics by differentiating loglik64 (float64 draws): G, H from l's derivative, T from tau's
    X64 = X.astype(np.float64)
    L = X64 @ w.T + b[:, g].T + o.astype(np.float64)[:, None]
    h = 1e-6
    R = (_per_row(fam, L + h, y, tau) - _per_row(fam, L - h, y, tau)) / (2 * h)
    ell = ref.loglik64(fam, L, y, tau)
    G = R.T @ X64
    H = np.zeros((S, J))
    np.add.at(H.T, g, R)
    T = (ref.loglik64(fam, L, y, tau + h) - ref.loglik64(fam, L, y, tau - h)) / (2 * h)
    _, grad = ref.elbo_and_grad(lam, eps, w, b, zeta, tau, ell, G, H, T, scale, prec, a0, b0, ga0, gb0)
    num = np.zeros(2 * P)
    for i in range(2 * P):
        e = np.zeros(2 * P)
        e[i] = 1e-5
        num[i] = (ref.elbo_fixed_draws(fam, lam + e, eps, X, y, g, J, scale, prec, a0, b0, ga0, gb0, o)
                  - ref.elbo_fixed_draws(fam, lam - e, eps, X, y, g, J, scale, prec, a0, b0, ga0, gb0, o)) / 2e-5
    npt.assert_allclose(grad, num, rtol=2e-6, atol=2e-6 * np.abs(num).max())


def _per_row(fam, L, y, tau):
    """loglik64's terms before the sum over the rows: [B, S]."""
    return np.stack([ref.loglik64(fam, L[n:n + 1], y[n:n + 1], tau) for n in range(L.shape[0])])


def test_noise_layout_and_draw():
    D, J, S = 4, 3, 5
    eps = ref.noise(D, J, S, 9, 2)
    assert eps.shape == (S, D + J + 2)
    npt.assert_array_equal(eps[:, :D + J + 1], ref.philox.normal_draws(9, S, D + J + 1, stream=0, step=2))
    npt.assert_array_equal(eps[:, -1:], ref.philox.normal_draws(9, S, 1, stream=1, step=2))
    lam = ref.init_lam(D + J + 2)
    W, Bm, zeta, logtau = ref.draw(lam, eps, D, J)
    assert W.shape == (S, D) and Bm.shape == (S, J) and zeta.dtype == np.float64 and logtau.dtype == np.float32
    npt.assert_allclose(zeta, 0.1 * eps[:, D + J])
    npt.assert_allclose(logtau, 0.1 * eps[:, D + J + 1], rtol=1e-6)


@pytest.fixture(scope="module")
def fits():
    out = {}
    for fam in FAMILIES:
        data = ref.simulate(fam)
        out[fam] = (data, ref.fit(fam, data, True), ref.fit(fam, data, False))
    return out


@pytest.mark.parametrize("fam", FAMILIES)
def test_simulated_fit_separates_the_models_with_room(fits, fam):
    """What tests/test_predict_scalar_group_gpu.py asserts on the device, in float64 and with a margin: known groups beat
    id -1, and the grouped model beats the family's ungrouped one, each by more than 0.05 nats per held-out row; the
    fitted intercept spread e^{-zeta / 2} is within a third of the simulated one."""
    data, lam, lam_flat = fits[fam]
    known = ref.heldout(fam, data, lam)
    new = ref.heldout(fam, data, lam, known=False)
    flat = ref.heldout(fam, data, lam_flat, grouped=False)
    P = ref.FIT["D"] + ref.FIT["J"] + 2
    spread = math.exp(-0.5 * lam[P - 2])
    print("%s: held-out lpd known %.4f, new groups %.4f, ungrouped %.4f; spread %.3f, e^tau %.3f" % (
        fam, known, new, flat, spread, math.exp(lam[P - 1])))
    assert known > new + 0.05
    assert known > flat + 0.05
    assert abs(spread - ref.FIT["spread"]) < ref.FIT["spread"] / 3.0


def test_constructor_refusals_that_need_no_device():
    from bayesic_amd.svi import HierGammaReparamSVI, HierNegBinReparamSVI, HierWeibullReparamSVI
    X, y, g = np.zeros((4, 8), np.float32), np.ones(4, np.float32), np.zeros(4, np.int32)
    for cls in (HierNegBinReparamSVI, HierGammaReparamSVI, HierWeibullReparamSVI):
        with pytest.raises(ValueError, match="mean-field guide only.*P = D \\+ J \\+ 2"):
            cls(X, y, g, 2, covariance="full")
        with pytest.raises(ValueError, match="n_groups must be an integer"):
            cls(X, y, g, 0)
        with pytest.raises(ValueError, match="group_a0 and group_b0"):
            cls(X, y, g, 2, group_b0=0.0)
        with pytest.raises(ValueError, match="a0 and b0"):
            cls(X, y, g, 2, a0=-1.0)
        with pytest.raises(ValueError, match="n_samples must be in"):
            cls(X, y, g, 2, n_samples=65)
    with pytest.raises(ValueError, match="finite and >= 0"):
        HierNegBinReparamSVI(X, -y, g, 2)
    with pytest.raises(ValueError, match="finite and > 0"):
        HierGammaReparamSVI(X, 0 * y, g, 2)
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        HierWeibullReparamSVI(X, -y, g, 2)
    with pytest.raises(ValueError, match="event must be a bool or 0/1"):
        HierWeibullReparamSVI(X, y, g, 2, event=np.array([0, 1, 2, 0]))
    with pytest.raises(NotImplementedError, match="not built"):
        HierWeibullReparamSVI(X, y, g, 2, upper=np.full(4, np.inf))
    with pytest.raises(ValueError, match="mutually exclusive"):
        HierNegBinReparamSVI(X, y, g, 2, offset=y, exposure=y)
    with pytest.raises(TypeError):
        HierWeibullReparamSVI(X, y, g, 2, exposure=y)
