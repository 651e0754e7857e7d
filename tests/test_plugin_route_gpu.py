"""the fused kernels reached THROUGH the plugin surface.  Config 2 is written with Normal /
InverseGamma nodes and bayesic.algebra expressions (inference/models.py), stepped by the general engine
ReparamVI; the engine recognises the data term with match (inference/recognise.py) and the update becomes
bsc_blr_data_pass + bsc_blr_fused_update_general -- equal to oracle.svi.blr_step on the same seed, bit-identical
to the hand-written driver svi/blr.py, and in the same time."""
import time

import numpy as np
import numpy.testing as npt
import pytest
import torch

from oracle import svi

pytestmark = pytest.mark.gpu


def _engine(ctx, X, y, scale, S, seed, lr, route="auto", order="W,xi", alpha0=1.0, beta0=1.0, lam0=None):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import linear_regression_log_joint
    lj, v = linear_regression_log_joint(scale, alpha0, beta0)
    D = X.shape[1]
    latents = [(v["W"], D), (v["xi"], 1)] if order == "W,xi" else [(v["xi"], 1), (v["W"], D)]
    return ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                     lam0=lam0, route=route)


def _lam_engine_order(lam_blr, D, order):
    m, rho, a, b = lam_blr[:D], lam_blr[D:2 * D], lam_blr[2 * D], lam_blr[2 * D + 1]
    if order == "W,xi":
        return np.concatenate([m, [a], rho, [b]])
    return np.concatenate([[a], m, [b], rho])


@pytest.mark.parametrize("order", ["W,xi", "xi,W"])
@pytest.mark.parametrize("D,S", [(256, 8), (64, 5)])
def test_config2_on_the_plugin_surface_equals_the_oracle_step(ctx, D, S, order):
    B, n_total, seed, lr = 6000, 60000.0, 1234, 0.01
    X, y, _ = svi.make_cfg2(B, D)
    lam = svi.blr_init_lam(D)
    eng = _engine(ctx, X, y, n_total / B, S, seed, lr, order=order, lam0=_lam_engine_order(lam, D, order))
    assert eng.route.startswith("fused"), eng.route
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in (1, 2, 3):
        assert eng.step() is None                     # asynchronous: nothing is read back inside a step
        lam, m1, m2, elbo, grad = svi.blr_step(lam, m1, m2, t, X, y, S, seed, n_total, lr)
        npt.assert_allclose(eng.elbo, elbo, rtol=1e-6)
        g, want = eng.grad, _lam_engine_order(grad, D, order)
        assert np.abs(g - want).max() <= 1e-4 * np.abs(want).max()
        npt.assert_allclose(eng.lam, _lam_engine_order(lam, D, order), atol=1e-4)
    assert eng.t == 3


def test_plugin_route_is_bit_identical_to_the_hand_written_driver(ctx):
    from bayesic_amd.svi.blr import BLRReparamSVI
    B, D, S = 20000, 256, 8
    X, y, _ = svi.make_cfg2(B, D)
    lam0 = svi.blr_init_lam(D)
    eng = _engine(ctx, X, y, 7.0, S, 99, 0.02, lam0=_lam_engine_order(lam0, D, "W,xi"))
    ref = BLRReparamSVI(X, y, n_total=7.0 * B, n_samples=S, seed=99, lr=0.02, ctx=ctx, lam0=lam0)
    for _ in range(4):
        eng.step()
        ref.step()
    ctx.sync()
    # the same two kernels on the same draws; the finish receives the model as five numbers fitted from the
    # symbolic log-joint instead of (scale, alpha0, beta0): equal to rounding of those numbers
    npt.assert_allclose(eng.lam, _lam_engine_order(ref.lam.cpu().numpy(), D, "W,xi"), rtol=1e-9, atol=1e-12)
    npt.assert_allclose(eng.elbo, ref.elbo.item(), rtol=1e-11)


def test_general_route_agrees_with_the_fused_route_in_expectation(ctx):
    """route='general' evaluates the expression as written (executor + autodiff, its own Philox layout): the two
    routes are different Monte-Carlo estimators of the same bound and gradient."""
    B, D, S = 4000, 32, 64
    X, y, _ = svi.make_cfg2(B, D)
    lam0 = _lam_engine_order(svi.blr_init_lam(D), D, "W,xi")
    fused = _engine(ctx, X, y, 3.0, S, 5, 1e-3, lam0=lam0)
    general = _engine(ctx, X, y, 3.0, S, 5, 1e-3, route="general", lam0=lam0)
    assert fused.route.startswith("fused") and general.route == "general"
    fused.step()
    general.step()
    ef, eg = fused.elbo, general.elbo
    assert abs(ef - eg) <= 0.02 * abs(eg), (ef, eg)
    gf, gg = fused.grad, general.grad
    cos = float(gf @ gg / (np.linalg.norm(gf) * np.linalg.norm(gg)))
    assert cos > 0.9, cos            # (two independent S = 64 estimates; the d/d rho half carries most of the noise)


def test_models_outside_the_family_take_the_general_route_and_fused_insists(ctx):
    from bayesic_amd import algebra as A
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    B, D, S = 3000, 16, 8
    X, y, _ = svi.make_cfg2(B, D)
    Xv, yv, W = A.var("X", 2), A.var("y", 1), A.var("W", 2)
    r = A.dimshuffle(yv, "x", 0) - A.dot(W, Xv.T)
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) + A.sum(W * W, axis=1) * (-0.5)      # known noise: no xi latent
    eng = ReparamVI(lj, [(W, D)], dict(X=X, y=y), n_samples=S, seed=3, backend=DeviceBackend(ctx))
    # the data term is recognised (ONE pass over X per step), the rest goes through the executor: the general route's
    # estimator on the general route's noise, so the two agree to float32 evaluation error
    assert eng.route.startswith("pass") and eng.plan is not None and eng.plan.family is None
    general = ReparamVI(lj, [(W, D)], dict(X=X, y=y), n_samples=S, seed=3, backend=DeviceBackend(ctx), route="general")
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        eng.step()
    finally:
        ctx.call = real_call
    general.step()
    assert calls.count("bsc_blr_data_pass_sweep") == 1      # the only launch that touches the data
    npt.assert_allclose(eng.elbo, general.elbo, rtol=1e-5)
    assert np.abs(eng.grad - general.grad).max() <= 1e-4 * np.abs(general.grad).max()
    npt.assert_allclose(eng.lam, general.lam, atol=1e-6)
    with pytest.raises(ValueError, match="family"):
        ReparamVI(lj, [(W, D)], dict(X=X, y=y), n_samples=S, backend=DeviceBackend(ctx), route="fused")


def test_shapes_the_pass_refuses_fall_back_to_the_general_route_with_the_reason(ctx):
    """the fused pass needs D % 4 == 0, a 16-byte aligned row-major X with a leading dimension % 4 == 0 and a
    contiguous y (check_pass_args, csrc/bsc_blr.hip).  route='auto' must see that BEFORE the first step and evaluate the
    model as written -- equal to the host backend's evaluation -- instead of raising BayesicHipError inside step()."""
    from oracle.einsum_eval import NumpyBackend
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import linear_regression_log_joint
    B, D, S = 2000, 6, 8
    X, y, _ = svi.make_cfg2(B, D)
    lj, v = linear_regression_log_joint(5.0, 1.0, 1.0)
    latents = [(v["W"], D), (v["xi"], 1)]
    eng = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=11, lr=1e-2, backend=DeviceBackend(ctx))
    assert eng.route == "general" and "multiple of 4" in eng.route_reason, (eng.route, eng.route_reason)
    with pytest.raises(ValueError, match="multiple of 4"):
        ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, backend=DeviceBackend(ctx), route="fused")
    # the same draws (the device's Philox) through the host backend: the same estimate
    eps = eng.draw(0)
    host = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=11, lr=1e-2, backend=NumpyBackend(np.float64),
                     noise=lambda step: eps)
    eng.step()
    host.step()
    npt.assert_allclose(eng.elbo, host.elbo, rtol=1e-5)
    assert np.abs(eng.grad - host.grad).max() <= 2e-4 * np.abs(host.grad).max()
    # a column-sliced view of a wider matrix: D = 8 is fine, the view is not the pass's layout either way it is run
    Xw_host = np.ascontiguousarray(np.random.RandomState(0).standard_normal((B, 13)).astype(np.float32))
    Xw = ctx.to_device(Xw_host)
    view = Xw[:, 1:9]                                    # stride 13, offset 4 bytes: neither % 4 nor 16-byte aligned
    latents2 = [(v["W"], 8), (v["xi"], 1)]
    eng2 = ReparamVI(lj, latents2, dict(X=view, y=ctx.to_device(y)), n_samples=S, seed=11, backend=DeviceBackend(ctx))
    assert eng2.route == "general" and "envelope" in eng2.route_reason
    # the general route must be RIGHT on the view, not merely finite: the host twin on the same draws and values
    eps2 = eng2.draw(0)
    host2 = ReparamVI(lj, latents2, dict(X=Xw_host[:, 1:9], y=y), n_samples=S, seed=11,
                      backend=NumpyBackend(np.float64), noise=lambda step: eps2)
    eng2.step()
    host2.step()
    npt.assert_allclose(eng2.elbo, host2.elbo, rtol=1e-5)
    assert np.abs(eng2.grad - host2.grad).max() <= 2e-4 * np.abs(host2.grad).max()


def test_set_data_with_another_row_count_is_refused_on_the_pass_route_too(ctx):
    """on the pass route (known noise variance: data term by the fused pass, the rest by the executor) every
    shape(X, 0) of the log-joint was resolved to a number when the model was recognised; another batch size would
    silently keep the old N in the normaliser terms."""
    from bayesic_amd import algebra as A
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    B, D, S = 3000, 16, 8
    X, y, _ = svi.make_cfg2(B, D)
    Xv, yv, W = A.var("X", 2), A.var("y", 1), A.var("W", 2)
    r = A.dimshuffle(yv, "x", 0) - A.dot(W, Xv.T)
    n_rows = A.shape(Xv, 0)
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) - n_rows * (0.5 * np.log(2 * np.pi * 0.25)) + A.sum(W * W, axis=1) * (-0.5)
    eng = ReparamVI(lj, [(W, D)], dict(X=X, y=y), n_samples=S, seed=3, backend=DeviceBackend(ctx))
    assert eng.route.startswith("pass")
    eng.step()
    before = eng.elbo
    X2, y2, _ = svi.make_cfg2(B, D)
    eng.set_data(X=X2 * 1.0, y=y2)                       # the same extent: accepted
    with pytest.raises(ValueError, match="planned for mini-batches of 3000 x 16"):
        eng.set_data(X=X[:2000], y=y[:2000])
    eng.step()                                           # the engine still holds a consistent batch
    assert np.isfinite(eng.elbo) and np.isfinite(before)


def test_plugin_route_runs_at_the_fused_drivers_speed(ctx):
    """<= 1.3 x the hand-written driver per update at 1M x 256, S = 8 (VERDICT r2 #1's bar; the two routes
    issue the same two launches, so the ratio is host overhead)."""
    from bayesic_amd.svi.blr import BLRReparamSVI
    B, D, S = 1_000_000, 256, 8
    g = torch.Generator(device=ctx.device).manual_seed(0)
    X = torch.randn((B, D), generator=g, device=ctx.device)
    y = torch.randn(B, generator=g, device=ctx.device)
    eng = _engine(ctx, X, y, 1.0, S, 1, 1e-3)
    ref = BLRReparamSVI(X, y, n_samples=S, seed=1, lr=1e-3, ctx=ctx)
    assert eng.route.startswith("fused")

    def per_step(model, steps=300):
        for _ in range(400):                      # past the start-up ramp
            model.step()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            model.step()
        ctx.sync()
        return (time.perf_counter() - t0) / steps

    t_ref = min(per_step(ref) for _ in range(2))
    t_eng = min(per_step(eng) for _ in range(2))
    print("plugin route %.1f us per update, hand-written driver %.1f us" % (t_eng * 1e6, t_ref * 1e6))
    assert t_eng <= 1.3 * t_ref, (t_eng, t_ref)
    assert t_eng <= 0.23e-3


# ---- config 3: the symbolic mixture model reaches csrc/bsc_mog.hip -------------------------------------

def test_symbolic_mixture_is_recognised_and_equals_the_oracle(ctx):
    """inference/mixture.py's model is a symbolic log-joint; route='auto' checks that the update rules match
    derived from it are the fused kernels' (recognise.diagonal_mixture) and runs those: equal to
    oracle.svi.mog_svi_step, bound included, with the prior read off the derived messages."""
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference.mixture import DiagonalMixtureVMP
    n, d, k = 50_000, 16, 64
    X, _, _ = svi.make_cfg3(n, d, k)
    prior = dict(alpha0=1.5, m0=0.1, kappa0=0.05, a0=2.0, b0=0.7)
    eta0 = svi.mog_prior_eta(k, d, **prior)
    eta = svi.mog_init_eta(X[:500], k, d, seed=2)
    alpha, m, kappa, a, b = svi.mog_unpack(eta, k, d)
    model = DiagonalMixtureVMP(X, k, n_total=10.0 * n, init=(alpha, m, kappa, a, b), backend=DeviceBackend(ctx), **prior)
    assert model.route.startswith("fused"), model.route
    derived = DiagonalMixtureVMP(X, k, n_total=10.0 * n, init=(alpha, m, kappa, a, b), backend=DeviceBackend(ctx),
                                 route="derived", **prior)
    for t in range(1, 4):
        rho = (t + 1.0) ** -0.6
        Wmat, c = svi.mog_expected_params(eta, k, d)
        _, lse = svi.mog_local_step(X, Wmat, c)
        want_elbo = svi.mog_elbo(eta, eta0, lse, 10.0, k, d)
        model.step(rho)
        derived.step(rho)
        eta, _, _ = svi.mog_svi_step(eta, eta0, X, 10.0 * n, rho, k, d)
        npt.assert_allclose(model.elbo(), want_elbo, rtol=2e-6)
        got = model.eta_fused_layout()
        scale = np.maximum(np.abs(eta), 1.0)
        assert (np.abs(got - eta) <= 1e-3 * scale).all(), np.abs((got - eta) / scale).max()   # (K = 64 overlapping components: float32 responsibilities feed back)
    # the node objects catch up on request: the derived engine's bound at the same state
    model.sync_nodes()
    derived.vmp.update("Z", 1.0, message_scale=1.0 / derived.scale)      # (sync_nodes leaves q(z) at its optimum for the new factors)
    derived_bound = derived.vmp.elbo()
    npt.assert_allclose(model.vmp.elbo(), derived_bound, rtol=1e-4)
    with pytest.raises(ValueError, match="MI355X backend"):
        from oracle.einsum_eval import NumpyBackend
        ones = np.ones((4, d))
        DiagonalMixtureVMP(X[:200].astype(np.float64), 4, init=(np.ones(4), 0.0 * ones, ones, ones, ones),
                           backend=NumpyBackend(np.float64), dtype="float64", resident=False, route="fused")


# ---- config 5: the score-function engine reaches csrc/bsc_bbvi.hip ---------------------------------------

def _config5_expression(D, G, scale, a0, b0):
    import math
    from bayesic_amd import algebra as A
    Xv, yv, Gm = A.var("X", 2), A.var("y", 1), A.var("Gm", 2)
    W, Bg, Z = A.var("W", 2), A.var("Bg", 2), A.var("Z", 2)          # [S, D], [S, G], [S, 1]
    L = A.dot(Xv, W.T) + A.dot(Gm, Bg.T)                              # logits [N, S]; the group of a row by a one-hot matrix
    loglik = A.sum(A.dimshuffle(yv, 0, "x") * L - A.log(1 + A.exp(L)), axis=0)
    zeta = A.sum(Z, axis=1)
    lp_w = A.sum(-0.5 * (W * W), axis=1) - 0.5 * D * math.log(2 * math.pi)
    lp_b = (-0.5 * G * math.log(2 * math.pi)) + (0.5 * G) * zeta - 0.5 * (A.exp(zeta) * A.sum(Bg * Bg, axis=1))
    lp_z = (a0 * math.log(b0) - math.lgamma(a0)) + a0 * zeta - b0 * A.exp(zeta)
    return scale * loglik + lp_w + lp_b + lp_z, [(W, D), (Bg, G), (Z, 1)]


def test_config5_on_the_plugin_surface_equals_the_oracle_step(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ScoreFunctionVI
    N, D, G, S = 6000, 16, 7, 64
    X, y, g, _, _ = svi.make_cfg5(N, D, G)
    n_total, lr, seed = 10.0 * N, 0.05, 5
    lj, latents = _config5_expression(D, G, n_total / N, 1.0, 1.0)
    data = {"X": X, "y": y, "Gm": np.eye(G, dtype=np.float32)[g]}
    eng = ScoreFunctionVI(lj, latents, data, n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx))
    assert eng.route.startswith("fused"), eng.route
    assert (eng.plan.scale, eng.plan.a0, eng.plan.b0) == pytest.approx((n_total / N, 1.0, 1.0), rel=1e-9)
    general = ScoreFunctionVI(lj, latents, data, n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                              route="general")
    P = D + G + 1
    lam = svi.bbvi_init_lam(P)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in (1, 2, 3):
        assert eng.step() is None
        general.step()
        lam, m1, m2, elbo, grad, ell = svi.bbvi_step(lam, m1, m2, t, X, y, g, D, G, S, seed, n_total, lr)
        npt.assert_allclose(eng.elbo, elbo, rtol=2e-6)
        gd = eng.grad
        assert np.abs(gd - grad).max() <= 2e-4 * np.abs(grad).max()
        npt.assert_allclose(eng.lam, lam, atol=2e-4)
        # the same draws on both routes: the general route's update is the same up to float32 evaluation
        npt.assert_allclose(general.elbo, eng.elbo, rtol=2e-5)
    # a group matrix that is not one-hot is not given an index vector
    bad = dict(data, Gm=data["Gm"] * 0.5)
    assert ScoreFunctionVI(lj, latents, bad, n_samples=S, backend=DeviceBackend(ctx)).route == "general"
    with pytest.raises(ValueError, match="one-hot"):
        ScoreFunctionVI(lj, latents, bad, n_samples=S, backend=DeviceBackend(ctx), route="fused")


def test_config5_plugin_route_runs_at_the_fused_drivers_speed(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ScoreFunctionVI
    from bayesic_amd.svi.bbvi import LogRegBBVI
    N, D, G, S = 1_000_000, 256, 1000, 64
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    X = torch.randn((N, D), generator=gen, device=ctx.device)
    y = (torch.rand(N, generator=gen, device=ctx.device) < 0.4).float()
    g = torch.randint(0, G, (N,), generator=gen, device=ctx.device, dtype=torch.int32)
    Gm = torch.zeros((N, G), device=ctx.device)
    Gm[torch.arange(N, device=ctx.device), g.long()] = 1.0
    lj, latents = _config5_expression(D, G, 1.0, 1.0, 1.0)
    eng = ScoreFunctionVI(lj, latents, {"X": X, "y": y, "Gm": Gm}, n_samples=S, seed=1, lr=1e-3, backend=DeviceBackend(ctx))
    assert eng.route.startswith("fused"), eng.route
    del Gm
    ref = LogRegBBVI(X, y, g, G, n_samples=S, seed=1, lr=1e-3, ctx=ctx)

    def per_step(model, steps=150):
        for _ in range(250):
            model.step()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            model.step()
        ctx.sync()
        return (time.perf_counter() - t0) / steps

    t_ref = min(per_step(ref) for _ in range(2))
    t_eng = min(per_step(eng) for _ in range(2))
    print("config 5: plugin route %.1f us per update, hand-written driver %.1f us" % (t_eng * 1e6, t_ref * 1e6))
    assert t_eng <= 1.3 * t_ref, (t_eng, t_ref)


@pytest.mark.parametrize("two_latents", [False, True])
def test_pass_route_with_its_state_on_the_device(two_latents):
    """A Gaussian-linear model one term away from config 2 (known noise: no xi latent; optionally a second latent the
    data term does not touch) takes the pass route; with resident=True draws, the ONE pass over X, the executor's walk of
    the parameter-sized surrogate, the d Q / d w = -2 G correction and Adam stay on the device, and from the third
    step on the whole step is a re-issued call list.  Same seed -> the host-side pass route's numbers."""
    from bayesic_amd import algebra as A
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.device import Context
    from bayesic_amd.inference import ReparamVI
    rs = np.random.RandomState(14)
    N, D, S = 30000, 24, 8
    Xs = rs.standard_normal((N, D)).astype(np.float32)
    ys = (Xs @ (rs.standard_normal(D) / 4) + 0.5 * rs.standard_normal(N)).astype(np.float32)
    X, y, W, c = A.var("X", 2), A.var("y", 1), A.var("W", 2), A.var("c", 2)
    r = A.dimshuffle(y, "x", 0) - A.dot(W, X.T)
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) + A.sum(W * W, axis=1) * (-0.5)
    latents = [(W, D)]
    if two_latents:
        lj = lj + A.sum(c * c, axis=1) * (-0.005)       # a latent that only the parameter-sized part mentions
        latents.append((c, 1))
    ctx = Context(0)
    engines = [ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, seed=9, backend=DeviceBackend(ctx), lr=0.02,
                         resident=resident) for resident in (False, True)]
    assert engines[0].route.startswith("pass") and engines[1].route.startswith("pass"), [e.route for e in engines]
    assert "resident" in engines[1].route and "resident" not in engines[0].route
    # ... and that is what route="auto" gives such a model unless told otherwise
    assert "resident" in ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, backend=DeviceBackend(ctx)).route
    crossings = []
    b1 = engines[1].backend
    real_to_host, real_sync = b1.to_host, ctx.sync
    b1.to_host = lambda value: (crossings.append("to_host"), real_to_host(value))[1]
    for step in range(8):
        host = engines[0].step()
        ctx.sync = lambda: (crossings.append("sync"), real_sync())[1]
        assert engines[1].step() is None
        ctx.sync = real_sync
        assert crossings == [], crossings
        assert abs(engines[1].elbo - host) <= 2e-6 * abs(host), (step, host, engines[1].elbo)
        scale = np.abs(engines[0].grad).max()
        npt.assert_allclose(engines[1].grad, engines[0].grad, rtol=0, atol=2e-5 * scale)
    npt.assert_allclose(engines[1].lam, engines[0].lam, rtol=0, atol=2e-4)
    (entry,) = [e for k, e in b1._replays.items() if k[0] == "reparam-step"]
    assert entry["calls"] is not None
    assert [call[2] for call in entry["calls"]].count("bsc_blr_data_pass_sweep") == 1     # one pass over the data
    walked = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (walked.append(name), real_call(name, *a))[1]
    engines[1].step()
    ctx.call = real_call
    assert sorted(walked) == ["bsc_adam_ascent", "bsc_adam_ascent", "bsc_philox_normal"], walked
    engines[0].step()
    # another mini-batch of the same shape: re-recorded, same numbers; another row count: refused (the surrogate holds N)
    Xs2 = rs.standard_normal((N, D)).astype(np.float32)
    for e in engines:
        e.set_data(X=Xs2)
    for step in range(4):
        host = engines[0].step()
        engines[1].step()
        assert abs(engines[1].elbo - host) <= 2e-6 * abs(host), (step, host, engines[1].elbo)
    with pytest.raises(ValueError):
        engines[1].set_data(X=Xs2[:1000], y=ys[:1000])


@pytest.mark.parametrize("two_latents", [False, True])
def test_general_reparam_engine_with_its_state_on_the_device(two_latents):
    """ReparamVI(route="general", resident=True): draws, z, the ELBO estimate, the pathwise gradient and the Adam
    step stay on the device (no host synchronisation inside step()); same seed -> the host-side engine's
    parameters, ELBO and gradient to float32 rounding of the [S, N] work, over several steps."""
    from bayesic_amd import algebra as A
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.device import Context
    from bayesic_amd.inference import ReparamVI
    rs = np.random.RandomState(4)
    N, D, S = 30000, 24, 8
    Xs = rs.standard_normal((N, D)).astype(np.float32)
    ys = (Xs @ (rs.standard_normal(D) / 4) + 0.7 + 0.5 * rs.standard_normal(N)).astype(np.float32)
    X, y, W, c = A.var("X", 2), A.var("y", 1), A.var("W", 2), A.var("c", 2)
    mean = A.dot(W, X.T)
    if two_latents:
        mean = mean + c                                 # [S, 1] intercept, broadcast over the rows
    r = A.dimshuffle(y, "x", 0) - mean
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) + A.sum(W * W, axis=1) * (-0.5)
    latents = [(W, D)]
    if two_latents:
        lj = lj + A.sum(c * c, axis=1) * (-0.005)
        latents.append((c, 1))
    ctx = Context(0)
    engines = [ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, seed=9, backend=DeviceBackend(ctx), lr=0.02,
                         route="general", resident=resident) for resident in (False, True)]
    assert "resident" in engines[1].route
    crossings = []
    b1 = engines[1].backend
    real_to_host, real_sync = b1.to_host, ctx.sync
    b1.to_host = lambda value: (crossings.append("to_host"), real_to_host(value))[1]
    for step in range(8):
        host = engines[0].step()
        ctx.sync = lambda: (crossings.append("sync"), real_sync())[1]
        assert engines[1].step() is None
        ctx.sync = real_sync
        assert crossings == [], crossings            # nothing read back, nothing waited for
        assert abs(engines[1].elbo - host) <= 2e-6 * abs(host), (step, host, engines[1].elbo)
        scale = np.abs(engines[0].grad).max()
        npt.assert_allclose(engines[1].grad, engines[0].grad, rtol=0, atol=2e-5 * scale)
    npt.assert_allclose(engines[1].lam, engines[0].lam, rtol=0, atol=2e-4)
    assert engines[1].t == engines[0].t == 8
    # from the third step on the resident engine re-issued a RECORDED list of C-ABI calls instead of walking the
    # expression (DeviceBackend.replay_call): the comparisons above ran on replayed steps
    (entry,) = [e for k, e in b1._replays.items() if k[0] == "reparam-step"]
    assert entry["calls"] is not None and len(entry["calls"]) >= 8
    walked = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (walked.append(name), real_call(name, *a))[1]
    engines[1].step()
    ctx.call = real_call
    assert sorted(walked) == ["bsc_adam_ascent", "bsc_adam_ascent", "bsc_philox_normal"], walked   # the rest came from the list
    engines[0].step()                                # (keep the two engines on the same step counter)
    # another mini-batch (new buffers): two eager steps, recorded again, and still the host engine's numbers
    Xs2 = rs.standard_normal((N, D)).astype(np.float32)
    for e in engines:
        e.set_data(X=Xs2)
    for step in range(5):
        host = engines[0].step()
        engines[1].step()
        assert abs(engines[1].elbo - host) <= 2e-6 * abs(host), (step, host, engines[1].elbo)
    (entry,) = [e for k, e in b1._replays.items() if k[0] == "reparam-step"]
    assert entry["calls"] is not None


def test_resident_reparam_engine_with_its_walk_recorded_as_a_graph():
    """resident=True and graph=True together: the draws are converted into fixed buffers, the walk is recorded on the
    third step and replayed; bit for bit the eager resident engine."""
    from bayesic_amd import algebra as A
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.device import Context
    from bayesic_amd.inference import ReparamVI
    rs = np.random.RandomState(6)
    N, D, S = 20000, 24, 8
    Xs = rs.standard_normal((N, D)).astype(np.float32)
    ys = (Xs @ (rs.standard_normal(D) / 4) + 0.5 * rs.standard_normal(N)).astype(np.float32)
    X, y, W = A.var("X", 2), A.var("y", 1), A.var("W", 2)
    r = A.dimshuffle(y, "x", 0) - A.dot(W, X.T)
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) + A.sum(W * W, axis=1) * (-0.5)
    prev = torch.cuda.current_stream()
    ctx = Context(0)
    ctx.set_stream(torch.cuda.Stream(ctx.device))
    try:
        engines = [ReparamVI(lj, [(W, D)], dict(X=Xs, y=ys), n_samples=S, seed=5, backend=DeviceBackend(ctx), lr=0.02,
                             route="general", resident=True, graph=graph) for graph in (False, True)]
        for step in range(10):
            engines[0].step()
            engines[1].step()
            assert engines[0].elbo == engines[1].elbo, step
            npt.assert_array_equal(engines[0].lam, engines[1].lam)
        entry = engines[1].backend._graphs[("reparam", id(engines[1]))]
        assert entry["graph"] is not None and not entry["dead"]         # it really was recorded
    finally:
        ctx.sync()
        torch.cuda.set_stream(prev)
        ctx.close()
