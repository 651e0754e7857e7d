"""GPU: the full-covariance Gaussian guide of the GLM path (bsc_glm_fullrank_update, GLMReparamSVI(covariance="full"),
ReparamVI(guide="full") on a recognised logistic / Poisson regression, posterior_draws) against the float64
restatement in tests/_glm_full_ref.py.

Tolerances (test_fullrank_gpu.py's, for the same arithmetic): the finish is float64 on both sides with the same inputs,
so lam_out, m1, m2, grad and the ELBO agree to rtol 1e-10 (absolute floor 1e-10 of the largest entry, for entries that
are sums with cancellation) and W_next within one float32 ulp; with a diagonal L the finish agrees with bsc_glm_update
to 1e-12; whole driver steps take the float32 data pass and use the existing five-step tolerance (ELBO rtol 1e-6, lam
atol 1e-4)."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

from oracle import philox, svi

import _glm_full_ref as ref

pytestmark = pytest.mark.gpu

ADAM = (0.9, 0.999, 1e-8)
SCALE, TAU, T, LR = 12.5, 0.7, 3, 0.01
WHO = "bsc_glm_fullrank_update"


def _inputs(D, S, seed, offdiag=0.05):
    """Random finish inputs with non-zero off-diagonal entries (offdiag = 0: a diagonal L).  eps and eps_next are in
    bsc_blr_noise's [S, D + 1] layout; column D is not read and holds a value that would show if it were."""
    r = np.random.RandomState(seed)
    L = np.tril(offdiag * r.standard_normal((D, D)), -1) + np.diag(np.exp(-2.0 + 0.3 * r.standard_normal(D)))
    lam = ref.pack(0.1 * r.standard_normal(D), L)
    n = lam.size
    m1 = 0.01 * r.standard_normal(n)
    m2 = 1e-4 * r.random_sample(n)
    eps = np.full((S, D + 1), 123.0)
    eps[:, :D] = r.standard_normal((S, D))
    W = ref.draw(lam, eps[:, :D])
    ell = -100.0 * r.uniform(1, 2, S)
    G = 5.0 * r.standard_normal((S, D))
    eps_next = np.full((S, D + 1), -77.0)
    eps_next[:, :D] = r.standard_normal((S, D))
    return dict(lam=lam, m1=m1, m2=m2, eps=eps, W=W, ell=ell, G=G, eps_next=eps_next)


def _device(ctx, inp):
    dev = lambda a, dt=torch.float64: ctx.to_device(np.ascontiguousarray(a), dt)
    S, D = inp["W"].shape
    return dict(stats=dev(np.concatenate([inp["ell"], inp["G"].reshape(-1)])), lam=dev(inp["lam"]),
                m1=dev(inp["m1"]), m2=dev(inp["m2"]), eps=dev(inp["eps"]), W=dev(inp["W"], torch.float32),
                eps_next=dev(inp["eps_next"]), W_next=ctx.zeros((S, D), torch.float32),
                elbo=ctx.zeros(1, torch.float64))


def _call(ctx, inp, ready=1, seed=7, next_step=4, name=WHO):
    """One finish (bsc_glm_fullrank_update, or bsc_glm_update on a mean-field lam); host copies of every output."""
    S, D = inp["W"].shape
    d = _device(ctx, inp)
    if not ready:
        d["eps_next"] = ctx.zeros((S, D + 1), torch.float64)
    lam_out, grad = ctx.zeros(inp["lam"].size, torch.float64), ctx.zeros(inp["lam"].size, torch.float64)
    ctx.call(name, d["stats"], d["lam"], lam_out, d["m1"], d["m2"], d["eps"], d["W"], D, S, SCALE, TAU, T, LR, *ADAM,
             seed, next_step, d["eps_next"], ready, d["W_next"], d["elbo"], grad)
    ctx.sync()
    npt.assert_array_equal(d["lam"].cpu().numpy(), inp["lam"])            # lam_in is not modified
    return dict(lam=lam_out.cpu().numpy(), m1=d["m1"].cpu().numpy(), m2=d["m2"].cpu().numpy(), grad=grad.cpu().numpy(),
                elbo=float(d["elbo"].item()), W_next=d["W_next"].cpu().numpy(), eps_next=d["eps_next"].cpu().numpy())


def _finish_ref(inp):
    D = inp["W"].shape[1]
    return ref.finish(inp["lam"], inp["m1"], inp["m2"], T, inp["eps"][:, :D], inp["W"], inp["ell"], inp["G"], SCALE, TAU,
                      LR)


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
    lam, m1, m2, elbo, grad = _finish_ref(inp)
    _close(out["lam"], lam, 1e-10)
    _close(out["m1"], m1, 1e-10)
    _close(out["m2"], m2, 1e-10)
    _close(out["grad"], grad, 1e-10)
    npt.assert_allclose(out["elbo"], elbo, rtol=1e-10)
    assert _ulps(out["W_next"], ref.draw(lam, inp["eps_next"][:, :D])) <= 1
    npt.assert_array_equal(out["eps_next"], inp["eps_next"])              # a ready eps_next is read, not drawn again


def test_kernel_draws_the_next_noise_when_it_is_not_ready(ctx):
    D, S = 100, 13
    inp = _inputs(D, S, seed=5)
    out = _call(ctx, inp, ready=0, seed=99, next_step=17)
    eps_next = ref.noise(D, S, 99, 17)
    npt.assert_allclose(out["eps_next"].reshape(S, D + 1)[:, :D], eps_next, rtol=1e-12, atol=1e-14)
    lam = _finish_ref(inp)[0]
    _close(out["lam"], lam, 1e-10)
    assert _ulps(out["W_next"], ref.draw(lam, eps_next)) <= 1


@pytest.mark.parametrize("D,S", [(8, 8), (256, 8), (100, 13)])
def test_diagonal_factor_reduces_to_the_mean_field_finish(ctx, D, S):
    """With every off-diagonal entry zero the ELBO, the mu / rho gradients and their Adam step are bsc_glm_update's on
    the same stats."""
    inp = _inputs(D, S, seed=3, offdiag=0.0)
    out = _call(ctx, inp)
    mf_inp = dict(inp, lam=ref.to_mean_field(inp["lam"], D), m1=ref.to_mean_field(inp["m1"], D),
                  m2=ref.to_mean_field(inp["m2"], D))
    mf_out = _call(ctx, mf_inp, name="bsc_glm_update")
    npt.assert_allclose(out["elbo"], mf_out["elbo"], rtol=1e-12)
    _close(ref.to_mean_field(out["grad"], D), mf_out["grad"], 1e-12)
    _close(ref.to_mean_field(out["lam"], D), mf_out["lam"], 1e-12)
    # (the next draws differ: the step gives the off-diagonal entries a gradient, so L' is no longer diagonal)


def test_two_identical_calls_give_identical_bytes(ctx):
    inp = _inputs(256, 64, seed=11)
    a, b = _call(ctx, inp), _call(ctx, inp)
    for k in ("lam", "m1", "m2", "grad", "W_next"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["elbo"] == b["elbo"]


def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    n = ref.n_lam(8)
    lam, m = ctx.zeros((2, n), f64), ctx.zeros((2, n), f64)
    eps, W = ctx.zeros((2, 65 * 9), f64), ctx.zeros((2, 65 * 8))
    stats, elbo, grad = ctx.zeros(65 * 9, f64), ctx.zeros(1, f64), ctx.zeros(n, f64)

    def call(D=8, S=8, lam_out=lam[1], eps_next=eps[1], W_next=W[1], tau=1.0, t=1):
        ctx.call(WHO, stats, lam[0], lam_out, m[0], m[1], eps[0], W[0], D, S, 1.0, tau, t, 0.01, *ADAM, 1, 1, eps_next, 1,
                 W_next, elbo, grad)

    with pytest.raises(BayesicHipError, match=WHO + ".*D=6 must be a multiple of 4"):
        call(D=6)
    with pytest.raises(BayesicHipError, match=WHO + ".*D=260"):
        call(D=260)
    with pytest.raises(BayesicHipError, match=WHO + ".*S=65"):
        call(S=65)
    with pytest.raises(BayesicHipError, match=WHO + ".*lam_in and lam_out must differ"):
        call(lam_out=lam[0])
    with pytest.raises(BayesicHipError, match=WHO + ".*must not alias"):
        call(eps_next=eps[0])
    with pytest.raises(BayesicHipError, match=WHO + ".*must not alias"):
        call(W_next=W[0])
    with pytest.raises(BayesicHipError, match=WHO + ".*both set or both null"):
        call(W_next=None)
    with pytest.raises(BayesicHipError, match=WHO + ".*prior_precision"):
        call(tau=0.0)
    with pytest.raises(BayesicHipError, match=WHO + ".*starts at 1"):
        call(t=0)
    ctx.sync()


def _cfg2_glm_data(link, B=4000, D=64):
    """X of svi.make_cfg2, y drawn from the link at the logits of make_cfg2's own w_true (standard deviation 0.5), as
    test_glm_gpu.py draws it from its logits."""
    X, _, w_true = svi.make_cfg2(B, D)
    l = X.astype(np.float64) @ w_true
    rs = np.random.RandomState(10)
    if link == "logistic":
        y = (rs.uniform(size=B) < 1.0 / (1.0 + np.exp(-l))).astype(np.float32)
    else:
        y = rs.poisson(np.exp(l)).astype(np.float32)
    return X, y


@pytest.mark.parametrize("S", [8, 16])
@pytest.mark.parametrize("link", ["logistic", "poisson"])
def test_driver_five_steps_match_the_restatement(ctx, link, S):
    from bayesic_amd.svi import GLMReparamSVI
    X, y = _cfg2_glm_data(link)
    D, seed, lr, n_total, tau = X.shape[1], 21, 0.02, 40000.0, 1.5
    model = GLMReparamSVI(X, y, link=link, n_total=n_total, n_samples=S, seed=seed, lr=lr, prior_precision=tau, ctx=ctx,
                          covariance="full")
    assert model.covariance_kind == "full"
    lam = ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 6):
        assert model.step() is None
        lam, m1, m2, elbo, grad = ref.step(link, lam, m1, m2, t, X, y, S, seed, n_total, lr, tau)
        ctx.sync()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=1e-4)
    p = model.params()
    assert p["L"].shape == (D, D) and (np.triu(p["L"], 1) == 0).all() and np.abs(np.tril(p["L"], -1)).max() > 0
    npt.assert_allclose(p["m"], lam[:D], atol=1e-4)
    npt.assert_allclose(p["rho"], np.log(np.diag(p["L"])), rtol=1e-12, atol=1e-14)
    npt.assert_allclose(model.covariance(), p["L"] @ p["L"].T, rtol=1e-14)
    with pytest.raises(ValueError, match="lam0 has 128 entries.*D = 64 needs 2144"):
        GLMReparamSVI(X, y, link=link, ctx=ctx, covariance="full", lam0=np.zeros(2 * D))
    diag = GLMReparamSVI(X, y, link=link, ctx=ctx)
    npt.assert_allclose(diag.covariance(), 0.01 * np.eye(D), rtol=1e-12)


def test_plugin_surface_takes_the_fused_full_rank_glm_route(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint
    from bayesic_amd.svi import GLMReparamSVI
    X, y = _cfg2_glm_data("logistic")
    B, D = X.shape
    S, seed, lr = 8, 1234, 0.01
    lj, v = logistic_regression_log_joint(7.0, 1.5)
    eng = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                    guide="full")
    assert eng.route == "fused: bsc_glm_data_pass + bsc_glm_fullrank_update (logistic link)", eng.route
    assert eng.route_reason is None and eng.lam.shape == (ref.n_lam(D),)
    # scale and tau as the recogniser fitted them from the symbolic log-joint: the same numbers reach the same kernels
    npt.assert_allclose([eng.plan.scale, eng.plan.tau], [7.0, 1.5], rtol=1e-9)
    model = GLMReparamSVI(X, y, link="logistic", n_total=eng.plan.scale * B, n_samples=S, seed=seed, lr=lr,
                          prior_precision=eng.plan.tau, ctx=ctx, covariance="full", lam0=eng.lam)
    for _ in range(3):
        assert eng.step() is None
        model.step()
    ctx.sync()
    npt.assert_array_equal(eng.lam, model.lam.cpu().numpy())
    assert eng.elbo == model.elbo.item()
    npt.assert_array_equal(eng.grad, model.grad.cpu().numpy())
    npt.assert_allclose(eng.covariance(), model.covariance(), rtol=1e-15)
    out = eng.predict(X, y)
    for k in ("mean", "var", "lpd"):
        assert out[k].shape == (B,) and bool(torch.isfinite(out[k]).all()), k
    # guide="diag" routes exactly as before
    diag = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx))
    assert diag.route == "fused: bsc_glm_data_pass + bsc_glm_update (logistic link)", diag.route


def test_posterior_draws_of_a_full_glm_model(ctx):
    from bayesic_amd.svi import GLMReparamSVI
    from bayesic_amd.svi import predict as mod
    X, y = _cfg2_glm_data("poisson", B=1000, D=16)
    D = X.shape[1]
    lam0 = _inputs(D, 1, seed=2, offdiag=0.1)["lam"]
    model = GLMReparamSVI(X, y, link="poisson", n_samples=8, seed=5, ctx=ctx, covariance="full", lam0=lam0)
    for S, seed in ((64, None), (5, 77)):
        W, lv = mod.posterior_draws(model, S, seed)
        assert lv is None and W.dtype == torch.float32 and tuple(W.shape) == (S, D)
        eps = philox.normal_draws(5 if seed is None else seed, S, D, stream=mod.PREDICT_STREAM, step=0)
        assert _ulps(W.cpu().numpy(), ref.draw(lam0, eps)) <= 1
    out = model.predict(X, y, n_samples=16)
    assert bool(torch.isfinite(out["mean"]).all()) and bool(torch.isfinite(out["lpd"]).all())


def posterior_covariance_errors(ctx, link, seed, steps=4000, D=8, B=2000, S=8, lr=1e-2):
    """Relative Frobenius error of Cov_q(w) (averaged over the second half of the steps) against the Laplace covariance
    H^{-1} at the MAP: (full guide, mean-field guide)."""
    from bayesic_amd.svi import GLMReparamSVI
    X, y = ref.ar_glm_design(link, B, D, seed)
    _, exact = ref.laplace(link, X, y)
    errs = []
    for cov in ("full", "diag"):
        model = GLMReparamSVI(X, y, link=link, n_samples=S, seed=seed, lr=lr, ctx=ctx, covariance=cov)
        acc = np.zeros((D, D))
        for t in range(1, steps + 1):
            model.step()
            if t > steps // 2:
                acc += model.covariance()
        errs.append(ref.covariance_error(acc / (steps - steps // 2), exact))
    return tuple(errs)


def test_full_guide_recovers_the_correlated_posterior_covariance(ctx):
    """D = 8, B = 2000, AR(0.9) design, logistic link, prior precision 1, 4000 steps of lr 1e-2 (seed 1), L L^T averaged
    over the second half, against the Laplace covariance at the MAP: the full guide's Cov(w) is close to it, the
    mean-field guide's is not.

    The float64 numpy restatement on the same Philox draws measures full 0.021 and mean-field 0.921
    (tests/test_glm_full_cpu.py); the device's own figures are printed by this test and have not been recorded from an
    MI355X run yet.  The thresholds are test_fullrank_gpu.py's."""
    full, diag = posterior_covariance_errors(ctx, "logistic", seed=1)
    print("full %.4f mean-field %.4f" % (full, diag))
    assert full <= 0.15, full
    assert diag >= 0.5, diag
