"""GPU: the full-covariance Gaussian guide (bsc_blr_fullrank_update, BLRReparamSVI(covariance="full"),
ReparamVI(guide="full")) against the float64 restatement in tests/_fullrank_ref.py.

Tolerances: the finish is float64 on both sides with the same inputs, so lam_out, m1, m2, grad and the ELBO agree to
rtol 1e-10 (absolute floor 1e-10 of the largest entry, for entries that are sums with cancellation), xi_next to
1e-12, W_next within one float32 ulp; whole driver steps take the float32 data pass and use the existing five-step
mean-field test's tolerance (ELBO rtol 1e-6, lam atol 1e-4)."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

from oracle import svi

import _fullrank_ref as ref

pytestmark = pytest.mark.gpu

ADAM = (0.9, 0.999, 1e-8)


def _inputs(D, S, seed, offdiag=0.05):
    """Random finish inputs with non-zero off-diagonal entries (offdiag = 0: a diagonal L)."""
    r = np.random.RandomState(seed)
    P = D + 1
    L = np.tril(offdiag * r.standard_normal((P, P)), -1) + np.diag(np.exp(-2.0 + 0.3 * r.standard_normal(P)))
    lam = ref.pack(0.1 * r.standard_normal(P), L)
    n = lam.size
    m1 = 0.01 * r.standard_normal(n)
    m2 = 1e-4 * r.random_sample(n)
    eps = r.standard_normal((S, P))
    W, xi = ref.draw(lam, eps)
    Q = 50.0 + 10.0 * r.random_sample(S)
    G = r.standard_normal((S, D))
    eps_next = r.standard_normal((S, P))
    family = (-120.0, -30.0, 2.0, 1.0, 1.0)
    return dict(lam=lam, m1=m1, m2=m2, eps=eps, W=W, xi=xi, Q=Q, G=G, eps_next=eps_next, family=family)


def _call(ctx, inp, t=3, lr=0.01, ready=1, seed=7, next_step=4):
    """One bsc_blr_fullrank_update; returns the host copies of every output."""
    D = inp["W"].shape[1]
    S = inp["W"].shape[0]
    dev = lambda a, dt=torch.float64: ctx.to_device(np.ascontiguousarray(a), dt)
    stats = dev(np.concatenate([inp["Q"], inp["G"].reshape(-1)]))
    lam_in, lam_out = dev(inp["lam"]), ctx.zeros(inp["lam"].size, torch.float64)
    m1, m2 = dev(inp["m1"]), dev(inp["m2"])
    eps, W, xi = dev(inp["eps"]), dev(inp["W"], torch.float32), dev(inp["xi"])
    eps_next = dev(inp["eps_next"]) if ready else ctx.zeros((S, D + 1), torch.float64)
    W_next, xi_next = ctx.zeros((S, D), torch.float32), ctx.zeros(S, torch.float64)
    elbo, grad = ctx.zeros(1, torch.float64), ctx.zeros(inp["lam"].size, torch.float64)
    ctx.call("bsc_blr_fullrank_update", stats, lam_in, lam_out, m1, m2, eps, W, xi, D, S, *inp["family"], t, lr,
             *ADAM, seed, next_step, eps_next, ready, W_next, xi_next, elbo, grad)
    ctx.sync()
    return dict(lam=lam_out.cpu().numpy(), m1=m1.cpu().numpy(), m2=m2.cpu().numpy(), grad=grad.cpu().numpy(),
                elbo=float(elbo.item()), W_next=W_next.cpu().numpy(), xi_next=xi_next.cpu().numpy(),
                eps_next=eps_next.cpu().numpy())


def _close(a, b, rtol):
    b = np.asarray(b, np.float64)
    npt.assert_allclose(a, b, rtol=rtol, atol=rtol * max(np.abs(b).max(), 1e-300))


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert (np.sign(a) == np.sign(b)).all() or np.abs(a - b).max() <= np.spacing(np.abs(b)).max()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("S", [1, 8, 13, 64])
@pytest.mark.parametrize("D", [4, 8, 100, 256])
def test_kernel_matches_the_restatement(ctx, D, S):
    inp = _inputs(D, S, seed=D * 100 + S)
    out = _call(ctx, inp)
    lam, m1, m2, elbo, grad = ref.finish(inp["lam"], inp["m1"], inp["m2"], 3, inp["eps"], inp["W"], inp["xi"],
                                         inp["Q"], inp["G"], inp["family"], 0.01)
    _close(out["lam"], lam, 1e-10)
    _close(out["m1"], m1, 1e-10)
    _close(out["m2"], m2, 1e-10)
    _close(out["grad"], grad, 1e-10)
    npt.assert_allclose(out["elbo"], elbo, rtol=1e-10)
    W_next, xi_next = ref.draw(lam, inp["eps_next"])
    npt.assert_allclose(out["xi_next"], xi_next, rtol=1e-12, atol=1e-12 * np.abs(xi_next).max())
    assert _ulps(out["W_next"], W_next) <= 1


def test_kernel_draws_the_next_noise_when_it_is_not_ready(ctx):
    D, S = 100, 13
    inp = _inputs(D, S, seed=5)
    out = _call(ctx, inp, ready=0, seed=99, next_step=17)
    npt.assert_allclose(out["eps_next"], ref.noise(D, S, 99, 17), rtol=1e-12, atol=1e-14)
    lam = ref.finish(inp["lam"], inp["m1"], inp["m2"], 3, inp["eps"], inp["W"], inp["xi"], inp["Q"], inp["G"],
                     inp["family"], 0.01)[0]
    W_next, xi_next = ref.draw(lam, ref.noise(D, S, 99, 17))
    npt.assert_allclose(out["xi_next"], xi_next, rtol=1e-12, atol=1e-12 * np.abs(xi_next).max())
    assert _ulps(out["W_next"], W_next) <= 1


@pytest.mark.parametrize("D,S", [(8, 8), (256, 8), (100, 13)])
def test_diagonal_factor_reduces_to_the_mean_field_finish(ctx, D, S):
    """With every off-diagonal entry zero the ELBO and the mu / rho gradients are bsc_blr_fused_update_general's on
    the same stats."""
    inp = _inputs(D, S, seed=3, offdiag=0.0)
    P = D + 1
    out = _call(ctx, inp)
    dslots = ref.diag_slots(P)
    rho = inp["lam"][dslots]
    mf = np.concatenate([inp["lam"][:D], rho[:D], [inp["lam"][D]], [rho[D]]])
    to_mf = lambda v: np.concatenate([v[:D], v[dslots][:D], [v[D]], [v[dslots][D]]])
    dev = lambda a, dt=torch.float64: ctx.to_device(np.ascontiguousarray(a), dt)
    stats = dev(np.concatenate([inp["Q"], inp["G"].reshape(-1)]))
    lam_in, lam_out = dev(mf), ctx.zeros(mf.size, torch.float64)
    m1, m2 = dev(to_mf(inp["m1"])), dev(to_mf(inp["m2"]))
    eps_next = dev(inp["eps_next"])
    W_next, xi_next = ctx.zeros((S, D), torch.float32), ctx.zeros(S, torch.float64)
    elbo, grad = ctx.zeros(1, torch.float64), ctx.zeros(mf.size, torch.float64)
    ctx.call("bsc_blr_fused_update_general", stats, lam_in, lam_out, m1, m2, dev(inp["eps"]),
             dev(inp["W"], torch.float32), dev(inp["xi"]), D, S, *inp["family"], 3, 0.01, *ADAM, 7, 4, eps_next, 1,
             W_next, xi_next, elbo, grad)
    ctx.sync()
    npt.assert_allclose(out["elbo"], elbo.item(), rtol=1e-12)
    _close(to_mf(out["grad"]), grad.cpu().numpy(), 1e-12)
    _close(to_mf(out["lam"]), lam_out.cpu().numpy(), 1e-12)
    # (the next draws differ: the step gives the off-diagonal entries a gradient, so L' is no longer diagonal)


def test_two_identical_calls_give_identical_bytes(ctx):
    inp = _inputs(256, 64, seed=11)
    a, b = _call(ctx, inp), _call(ctx, inp)
    for k in ("lam", "m1", "m2", "grad", "W_next", "xi_next"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["elbo"] == b["elbo"]


def _driver_vs_restatement(ctx, X, y, S, seed, lr, n_total, steps=5, **kw):
    from bayesic_amd.svi.blr import BLRReparamSVI
    model = BLRReparamSVI(X, y, n_total=n_total, n_samples=S, seed=seed, lr=lr, ctx=ctx, covariance="full", **kw)
    D = X.shape[1]
    lam = ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, steps + 1):
        model.step()
        lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, X, y, S, seed, n_total, lr)
        ctx.sync()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=1e-4)
    return model


def test_driver_five_steps_match_the_restatement(ctx):
    X, y, _ = svi.make_cfg2(4000, 64)
    m8 = _driver_vs_restatement(ctx, X, y, 8, 21, 0.02, 40000.0)
    m16 = _driver_vs_restatement(ctx, X, y, 16, 21, 0.02, 40000.0)
    rep = _driver_vs_restatement(ctx, X, y, 16, 21, 0.02, 40000.0, reproducible=True)
    npt.assert_allclose(rep.lam.cpu().numpy(), m16.lam.cpu().numpy(), atol=1e-4)
    npt.assert_allclose(rep.elbo.item(), m16.elbo.item(), rtol=1e-6)
    p = m8.params()
    assert p["L"].shape == (65, 65) and (np.triu(p["L"], 1) == 0).all()
    npt.assert_allclose(m8.covariance(), p["L"] @ p["L"].T, rtol=1e-14)


def test_plugin_surface_takes_the_fused_full_rank_route(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import linear_regression_log_joint
    from bayesic_amd.svi.blr import BLRReparamSVI
    B, D, S, seed = 6000, 256, 8, 1234
    X, y, _ = svi.make_cfg2(B, D)
    lj, v = linear_regression_log_joint(10.0, 1.0, 1.0)
    eng = ReparamVI(lj, [(v["W"], D), (v["xi"], 1)], dict(X=X, y=y), n_samples=S, seed=seed, lr=0.01,
                    backend=DeviceBackend(ctx), guide="full")
    assert eng.route == "fused: bsc_blr_data_pass + bsc_blr_fullrank_update", eng.route
    model = BLRReparamSVI(X, y, n_samples=S, seed=seed, lr=0.01, ctx=ctx, lam0=eng.lam, family=eng.plan.family[:5],
                          covariance="full")
    for _ in range(3):
        eng.step()
        model.step()
    npt.assert_array_equal(eng.lam, model.lam.cpu().numpy())
    assert eng.elbo == model.elbo.item()
    npt.assert_array_equal(eng.grad, model.grad.cpu().numpy())
    npt.assert_allclose(eng.covariance(), model.covariance(), rtol=1e-15)
    # the same model with the scale latent listed first: the triangular factor is tied to [w | xi], so the general route
    xi_first = ReparamVI(lj, [(v["xi"], 1), (v["W"], D)], dict(X=X[:64], y=y[:64]), n_samples=S, seed=seed,
                         backend=DeviceBackend(ctx), guide="full")
    assert not xi_first.route.startswith("fused") and "weights first" in xi_first.route_reason


def _ar_design(B, D, seed, noise_sd):
    """AR(0.9) features with unit marginal variance: neighbouring columns correlated 0.9, the posterior of w with them."""
    r = np.random.RandomState(seed)
    X = np.empty((B, D))
    X[:, 0] = r.standard_normal(B)
    for d in range(1, D):
        X[:, d] = 0.9 * X[:, d - 1] + math.sqrt(1.0 - 0.81) * r.standard_normal(B)
    y = X @ (r.standard_normal(D) / 2.0) + noise_sd * r.standard_normal(B)
    return X.astype(np.float32), y.astype(np.float32)


NOISE_SD = 1.0


def posterior_covariance_errors(ctx, seed, steps=4000, D=8, B=2000, S=8, lr=1e-2):
    """Relative Frobenius error of the w block of Cov_q (averaged over the second half of the steps) against the exact
    Normal-Inverse-Gamma posterior covariance b_n / (a_n - 1) Lambda_n^{-1}: (full guide, mean-field guide)."""
    from bayesic_amd.svi.blr import BLRReparamSVI
    X, y = _ar_design(B, D, seed, NOISE_SD)
    _, Lam, a_n, b_n = svi.blr_exact_posterior(X, y)
    exact = b_n / (a_n - 1.0) * np.linalg.inv(Lam)
    errs = []
    for cov in ("full", "diag"):
        model = BLRReparamSVI(X, y, n_samples=S, seed=seed, lr=lr, ctx=ctx, covariance=cov)
        acc = np.zeros((D + 1, D + 1))
        for t in range(1, steps + 1):
            model.step()
            if t > steps // 2:
                acc += model.covariance()
        C = acc[:D, :D] / (steps - steps // 2)
        errs.append(float(np.linalg.norm(C - exact) / np.linalg.norm(exact)))
    return tuple(errs)


def test_full_guide_recovers_the_correlated_posterior_covariance(ctx):
    """D = 8, B = 2000, AR(0.9) design, 4000 steps of lr 1e-2, L L^T averaged over the second half: the full guide's
    Cov(w) is close to the exact posterior covariance, the mean-field guide's is not.

    Measured on MI355X (noise sd 1.0, S = 8; seeds 1, 2, 3): full 0.036, 0.045, 0.032; mean-field 0.926, 0.927,
    0.927 (the float64 numpy restatement: 0.036 and 0.045 for seeds 1 and 2).  The tolerances leave the full guide
    a 3x margin and are far from the mean-field guide's error, which no number of steps reduces."""
    full, diag = posterior_covariance_errors(ctx, seed=1)
    assert full <= 0.15, full
    assert diag >= 0.5, diag
