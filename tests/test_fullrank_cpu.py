"""The full-covariance Gaussian guide on the host (no GPU): ReparamVI(guide="full") on the float64 numpy backend
against the restatement in tests/_fullrank_ref.py, its reduction to the mean-field guide, and argument checks."""
import numpy as np
import numpy.testing as npt
import pytest

from oracle.einsum_eval import NumpyBackend

import _fullrank_ref as ref

B64 = NumpyBackend(np.float64)


def _config2(N=64, D=4, scale=5.0, seed=3):
    """Config 2 on the plugin surface in float64: (log-joint, latents [W, xi], data, family)."""
    from bayesic_amd.inference.models import linear_regression_log_joint
    r = np.random.RandomState(seed)
    X = r.standard_normal((N, D))
    y = X @ (r.standard_normal(D) / 4.0) + 0.5 * r.standard_normal(N)
    lj, v = linear_regression_log_joint(scale, 1.0, 1.0, dtype="float64")
    return lj, [(v["W"], D), (v["xi"], 1)], dict(X=X, y=y), ref.nig_family(N, scale, D)


def _noise(S, P):
    return lambda step: np.random.RandomState(100 + step).standard_normal((S, P))


def _lam0(D, seed=11):
    """A full-layout lam with non-zero off-diagonal entries."""
    P = D + 1
    r = np.random.RandomState(seed)
    L = np.tril(0.05 * r.standard_normal((P, P)), -1) + np.diag(np.exp(np.full(P, np.log(0.1)) + 0.1 * r.standard_normal(P)))
    return ref.pack(0.1 * r.standard_normal(P), L)


def test_full_guide_on_the_host_matches_the_restatement_over_five_steps():
    from bayesic_amd.inference import ReparamVI
    D, S = 4, 6
    P = D + 1
    lj, latents, data, family = _config2(D=D)
    noise = _noise(S, P)
    lam0 = _lam0(D)
    eng = ReparamVI(lj, latents, data, n_samples=S, backend=B64, lr=0.01, lam0=lam0, noise=noise, guide="full")
    assert eng.route == "general" and eng.lam.shape == (ref.n_lam(D),)
    X, y = data["X"], data["y"]
    lam, m1, m2 = lam0.copy(), np.zeros_like(lam0), np.zeros_like(lam0)
    for t in range(1, 6):
        elbo = eng.step()
        eps = noise(t - 1)
        mu, L = ref.unpack(lam, P)
        z = mu[None, :] + eps @ L.T
        W, xi = z[:, :D], z[:, D]
        R = y[None, :] - W @ X.T
        f, g = ref.family_f_and_g(W, xi, (R * R).sum(axis=1), R @ X, family)
        elbo_ref, grad = ref.estimate(lam, eps, f, g)
        lam, m1, m2 = ref.svi.adam_ascent(lam, grad, m1, m2, t, 0.01)
        npt.assert_allclose(elbo, elbo_ref, rtol=1e-12)
        npt.assert_allclose(eng.grad, grad, rtol=1e-12, atol=1e-12 * np.abs(grad).max())
        npt.assert_allclose(eng.lam, lam, rtol=1e-12, atol=1e-14)
    mu, L = ref.unpack(lam, P)
    npt.assert_allclose(eng.covariance(), L @ L.T, rtol=1e-12, atol=1e-16)
    assert (np.abs(np.triu(eng.unpack()[1], 1)) == 0).all()


def test_full_guide_with_a_diagonal_factor_is_the_mean_field_step():
    """Zero off-diagonal entries: one step's ELBO and its mu / rho gradients equal guide="diag"'s on the same noise."""
    from bayesic_amd.inference import ReparamVI
    D, S = 4, 8
    P = D + 1
    lj, latents, data, _ = _config2(D=D, seed=5)
    r = np.random.RandomState(2)
    mf = np.concatenate([0.2 * r.standard_normal(P), np.log(0.1) + 0.2 * r.standard_normal(P)])
    full = np.zeros(ref.n_lam(D))
    full[:P], full[ref.diag_slots(P)] = mf[:P], mf[P:]
    noise = _noise(S, P)
    diag = ReparamVI(lj, latents, data, n_samples=S, backend=B64, lr=0.01, lam0=mf, noise=noise)
    fr = ReparamVI(lj, latents, data, n_samples=S, backend=B64, lr=0.01, lam0=full, noise=noise, guide="full")
    e_d, g_d = diag.estimate(0)
    e_f, g_f = fr.estimate(0)
    npt.assert_allclose(e_f, e_d, rtol=1e-12)
    npt.assert_allclose(g_f[:P], g_d[:P], rtol=1e-12)
    npt.assert_allclose(g_f[ref.diag_slots(P)], g_d[P:], rtol=1e-12)
    npt.assert_allclose(fr.covariance(), diag.covariance(), rtol=1e-12)


def test_bad_guide_or_covariance_is_refused():
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.svi.blr import BLRReparamSVI
    lj, latents, data, _ = _config2()
    with pytest.raises(ValueError, match="guide"):
        ReparamVI(lj, latents, data, n_samples=4, backend=B64, guide="lowrank")
    with pytest.raises(ValueError, match="covariance"):
        BLRReparamSVI(np.zeros((8, 4), np.float32), np.zeros(8, np.float32), covariance="dense")


def test_restatement_layout_round_trips():
    D = 8
    lam = _lam0(D)
    mu, L = ref.unpack(lam, D + 1)
    npt.assert_allclose(ref.pack(mu, L), lam, rtol=1e-15, atol=1e-15)
    assert ref.n_lam(256) == 33410
