"""GPU parity of the GLM path (csrc/bsc_glm.hip through the C ABI, svi/glm.py, the plugin route) against the float64
restatement in tests/_glm_ref.py.

Tolerances (the project's existing ones for the same arithmetic: float32 operands, float32 products and per-lane
partial sums, float64 finish):
 * ell: |dev - ref| <= 2e-5 * sum_n (|y_n l_ns| + A(l_ns) + 1)      (test_bbvi_gpu's bound for its log-likelihood);
 * G: rtol 1e-4, atol 1e-4 * max|G|                                  (test_blr_gpu's for the leading-dimension pass);
 * the finish from given statistics (float64 both sides): rtol 1e-9  (test_bbvi_gpu, parameter side);
 * several updates against the reference: ELBO rtol 1e-6, gradient 1e-4 * max|grad|, lam atol 2e-4
   (test_blr_gpu.test_full_update_steps_track_the_oracle).
Poisson inputs keep |l| <= 4 (asserted on the float64 logits)."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_ref as ref

pytestmark = pytest.mark.gpu

LINKS = ("logistic", "poisson")
CODE = {"logistic": 0, "poisson": 1}


def _pass(ctx, link, X, y, W, ld=None):
    """bsc_glm_data_pass on host arrays; ``ld``: X is handed over inside a wider buffer of that leading dimension."""
    B, D = X.shape
    S = W.shape[0]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    yd, Wd = ctx.to_device(y), ctx.to_device(W)
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    ctx.call("bsc_glm_data_pass", CODE[link], Xd, (ld or D), yd, B, D, Wd, S, ell, G)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy()


def _inputs(link, B, D, S, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    if link == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        # Poisson inputs keep |l| <= 4: the draws are shrunk where a heavy-tailed narrow design would exceed it
        peak = np.abs(X.astype(np.float64) @ W.astype(np.float64).T).max() if B else 0.0
        if peak > 3.5:
            W = (W * (3.5 / peak)).astype(np.float32)
    return X, y, W


def _check_pass(ctx, link, X, y, W, ld=None):
    ell, G = _pass(ctx, link, X, y, W, ld)
    ell_r, G_r = ref.glm_data_pass(link, X, y, W)
    L = X.astype(np.float64) @ W.astype(np.float64).T
    if link == "poisson":
        assert np.abs(L).max() <= 4.0 if L.size else True
    A, _ = ref.log_partition(link, L)
    bound = (np.abs(y.astype(np.float64)[:, None] * L) + A + 1.0).sum(axis=0)
    err = np.abs(ell - ell_r)
    print("%s B=%d D=%d S=%d: ell err/bound %.3g, G err/max %.3g" % (
        link, X.shape[0], X.shape[1], W.shape[0], (err / (bound + 1e-300)).max(),
        np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300)))
    assert (err <= 2e-5 * bound + 1e-12).all(), (err / (bound + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    return ell, G


@pytest.mark.parametrize("S", [1, 3, 8, 9, 16, 64])
@pytest.mark.parametrize("B,D", [(0, 256), (5, 256), (32, 256), (1003, 256), (20000, 252), (4099, 64), (777, 4)])
@pytest.mark.parametrize("link", LINKS)
def test_pass_matches_the_reference(ctx, link, B, D, S):
    X, y, W = _inputs(link, B, D, S, seed=B * 7 + D + S)
    ell, G = _check_pass(ctx, link, X, y, W)
    if B == 0:
        assert (ell == 0).all() and (G == 0).all()


@pytest.mark.parametrize("B,D,ld", [(333, 64, 96), (1003, 256, 260), (50, 256, 512)])
@pytest.mark.parametrize("link", LINKS)
def test_pass_respects_the_leading_dimension(ctx, link, B, D, ld):
    X, y, W = _inputs(link, B, D, 8, seed=ld)
    _check_pass(ctx, link, X, y, W, ld=ld)


def test_pass_with_a_y_that_is_not_16_byte_aligned_takes_the_other_kernel(ctx):
    """D = 256 with y starting 4 bytes into its buffer: the 8-row kernel (the MFMA kernel loads y 16 bytes at a time)."""
    X, y, W = _inputs("logistic", 1003, 256, 8, seed=3)
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    ybuf = ctx.to_device(np.concatenate([[9.0], y]).astype(np.float32))
    ell, G = ctx.zeros(8, torch.float64), ctx.zeros((8, 256), torch.float64)
    ctx.call("bsc_glm_data_pass", 0, Xd, 256, ybuf[1:], 1003, 256, Wd, 8, ell, G)
    ctx.sync()
    ell_r, G_r = ref.glm_data_pass("logistic", X, y, W)
    npt.assert_allclose(ell.cpu().numpy(), ell_r, rtol=2e-5)
    npt.assert_allclose(G.cpu().numpy(), G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("link", LINKS)
def test_operand_layout_with_exact_integers(ctx, link, D):
    """One-hot rows (row n has a single 1 in column 3 n mod D) and draws that look at the columns d = s mod 8 with
    weight s + 1: l[n, s] is s + 1 or 0, row n lands in exactly one column of G, and which rows count for which draw changes
    with any mix-up of the row, draw or column mapping (ell) or of the accumulator layout (G).  The bounds: float32
    exp / log1p at 1 ulp on sums of <= 96 terms (ell, rtol 1e-6); 1 - sigmoid(l) is formed at ulp(1) (G, atol 2e-7)."""
    B, S = (96, 8) if D == 256 else (20, 8)
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), (3 * np.arange(B)) % D] = 1.0
    W = np.zeros((S, D), np.float32)
    for s in range(S):
        W[s, s::8] = s + 1.0
    y = (np.arange(B) % 3 == 0).astype(np.float32)
    ell, G = _pass(ctx, link, X, y, W)
    ell_r, G_r = ref.glm_data_pass(link, X, y, W)
    npt.assert_allclose(ell, ell_r, rtol=1e-6)
    npt.assert_allclose(G, G_r, rtol=1e-6, atol=2e-7 if link == "logistic" else 0.0)
    assert len(set(np.round(ell_r, 3))) > 4 and len(set(np.round(G_r.ravel(), 4))) > 2


@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
def test_logistic_at_extreme_logits(ctx, D, B):
    """l = +-80: exp(80) overflows float32, the stable softplus / sigmoid do not."""
    S = 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(D)[None, :])
    W = (80.0 * sign).astype(np.float32)
    y = ((np.arange(B) // 2) % 2).astype(np.float32)
    ell, G = _pass(ctx, "logistic", X, y, W)
    assert np.isfinite(ell).all() and np.isfinite(G).all()
    ell_r, G_r = ref.glm_data_pass("logistic", X, y, W)
    L = X.astype(np.float64) @ W.astype(np.float64).T
    assert set(np.unique(L)) == {-80.0, 80.0}
    npt.assert_allclose(ell, ell_r, rtol=1e-6)
    npt.assert_allclose(G, G_r, rtol=1e-6)


def test_refusals_name_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9), ctx.zeros((65, 260))
    ell, G = ctx.zeros(65, torch.float64), ctx.zeros((65, 260), torch.float64)

    def call(link, Xa, ldx, D, S):
        ctx.call("bsc_glm_data_pass", link, Xa, ldx, y, 8, D, W, S, ell, G)

    with pytest.raises(BayesicHipError, match="D=6 must be a multiple of 4"):
        call(0, X, 8, 6, 8)
    with pytest.raises(BayesicHipError, match="D=260 must be a multiple of 4 in"):
        call(0, X, 260, 260, 8)
    with pytest.raises(BayesicHipError, match="16-byte aligned"):
        call(0, X.view(-1)[1:], 256, 256, 8)                # X offset by 4 bytes
    with pytest.raises(BayesicHipError, match="S=65"):
        call(1, X, 256, 256, 65)
    with pytest.raises(BayesicHipError, match="link=2"):
        call(2, X, 256, 256, 8)
    with pytest.raises(BayesicHipError, match="ldx=6"):
        call(0, X, 6, 8, 8)
    lam, m = ctx.zeros((2, 16), torch.float64), ctx.zeros((2, 16), torch.float64)
    eps = ctx.zeros((2, 8 * 9), torch.float64)
    with pytest.raises(BayesicHipError, match="S=9"):        # the one-call form takes eight draws
        ctx.call("bsc_glm_pass_update", 0, X, 8, y, 8, 8, lam[0], lam[1], m[0], m[1], eps[0], W, 9, 1.0, 1.0, 1, 0.01,
                 0.9, 0.999, 1e-8, 1, 1, eps[1], 1, W, ell, G)
    with pytest.raises(BayesicHipError, match="prior_precision"):
        ctx.call("bsc_glm_update", G, lam[0], lam[1], m[0], m[1], eps[0], W, 8, 8, 1.0, 0.0, 1, 0.01, 0.9, 0.999, 1e-8,
                 1, 1, None, 0, None, ell, G)
    ctx.sync()


@pytest.mark.parametrize("link", LINKS)
def test_pass_is_deterministic(ctx, link):
    X, y, W = _inputs(link, 5000, 256, 16, seed=5)
    a = _pass(ctx, link, X, y, W)
    b = _pass(ctx, link, X, y, W)
    npt.assert_array_equal(a[0], b[0])
    npt.assert_array_equal(a[1], b[1])


@pytest.mark.parametrize("D,S,ready", [(24, 5, 1), (20, 16, 1), (256, 8, 0)])
def test_finish_from_given_statistics(ctx, D, S, ready):
    """bsc_glm_update(stats): float64 on both sides."""
    rs = np.random.RandomState(D + S)
    f64 = torch.float64
    lam = np.concatenate([0.2 * rs.standard_normal(D), math.log(0.1) + 0.1 * rs.standard_normal(D)])
    m1, m2 = 0.01 * rs.standard_normal(2 * D), 1e-4 * rs.uniform(size=2 * D)
    ell, G = -100.0 * rs.uniform(1, 2, S), rs.standard_normal((S, D)) * 5
    seed, t, scale, tau, lr = 99, 4, 12.5, 0.7, 0.02
    eps = np.zeros((S, D + 1))
    eps[:, :D] = ref.noise(D, S, seed, t - 1)
    eps[:, D] = 123.0                                      # the scalar latent's column of the layout is not read
    W = ref.draw(lam, eps[:, :D])
    eps_n = np.zeros((S, D + 1))
    eps_n[:, :D] = ref.noise(D, S, seed, t)
    d = dict(stats=ctx.to_device(np.concatenate([ell, G.ravel()]), f64), lam=ctx.to_device(lam, f64),
             out=ctx.zeros(2 * D, f64), m1=ctx.to_device(m1, f64), m2=ctx.to_device(m2, f64),
             eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()),
             eps_n=ctx.to_device(eps_n.ravel() if ready else np.zeros(S * (D + 1)), f64), W_n=ctx.zeros(S * D),
             elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * D, f64))
    ctx.call("bsc_glm_update", d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], D, S, scale, tau, t,
             lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], ready, d["W_n"], d["elbo"], d["grad"])
    ctx.sync()
    lam_r, m1_r, m2_r, elbo_r, grad_r = ref.finish(lam, m1, m2, t, eps[:, :D], W, ell, G, scale, tau, lr)
    npt.assert_allclose(d["elbo"].item(), elbo_r, rtol=1e-9)
    npt.assert_allclose(d["grad"].cpu().numpy(), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
    npt.assert_allclose(d["out"].cpu().numpy(), lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(d["m1"].cpu().numpy(), m1_r, rtol=1e-9, atol=1e-15)
    npt.assert_allclose(d["m2"].cpu().numpy(), m2_r, rtol=1e-9, atol=1e-18)
    npt.assert_allclose(d["lam"].cpu().numpy(), lam, rtol=0, atol=0)       # lam_in is not modified
    npt.assert_allclose(d["eps_n"].cpu().numpy().reshape(S, D + 1)[:, :D], eps_n[:, :D], rtol=1e-12, atol=1e-14)
    # the next draw: float32-rounded from float64 on both sides (1 ulp where the float64 values straddle a tie)
    npt.assert_allclose(d["W_n"].cpu().numpy().reshape(S, D), ref.draw(lam_r, eps_n[:, :D]), rtol=2e-7, atol=1e-9)


def _regression_data(link, B, D, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    L = X.astype(np.float64) @ rs.standard_normal(D)
    if link == "logistic":
        y = (rs.uniform(size=B) < 1.0 / (1.0 + np.exp(-L))).astype(np.float32)
    else:
        y = rs.poisson(np.exp(L)).astype(np.float32)
    return X, y


@pytest.mark.parametrize("S", [8, 16])            # the one-call path / data pass -> all-reduce -> finish(stats)
@pytest.mark.parametrize("link", LINKS)
def test_twenty_updates_track_the_reference_over_two_batches(ctx, link, S):
    from bayesic_amd.svi import GLMReparamSVI
    B, D, seed, lr, tau = 3000, 256, 1234, 0.01, 2.0
    batches = [_regression_data(link, B, D, 10 + k) for k in range(2)]
    dev = [(ctx.to_device(X), ctx.to_device(y)) for X, y in batches]
    model = GLMReparamSVI(dev[0][0], dev[0][1], link=link, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr,
                          prior_precision=tau, ctx=ctx)
    lam = ref.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 21):
            k = (t - 1) % 2
            model.set_batch(*dev[k])
            assert model.step() is None
            lam, m1, m2, elbo, grad = ref.glm_step(link, lam, m1, m2, t, batches[k][0], batches[k][1], S, seed,
                                                   10.0 * B, lr, tau)
            if t in (1, 2, 3, 10, 20):
                ctx.sync()
                g = model.grad.cpu().numpy()
                npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert ("bsc_glm_pass_update" in calls) == (S == 8) and ("bsc_glm_update" in calls) == (S == 16)
    p = model.params()
    npt.assert_allclose(np.concatenate([p["m"], p["rho"]]), lam, atol=2e-4)


def test_the_driver_is_deterministic(ctx):
    from bayesic_amd.svi import GLMReparamSVI
    X, y = _regression_data("poisson", 4099, 64, 1)
    out = []
    for _ in range(2):
        model = GLMReparamSVI(X, y, link="poisson", n_total=40990, n_samples=8, seed=7, lr=0.02, ctx=ctx)
        for _ in range(4):
            model.step()
        ctx.sync()
        out.append((model.lam.cpu().numpy().copy(), model.elbo.item()))
    npt.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def test_the_plugin_surface_reaches_the_fused_glm_route(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint, poisson_regression_log_joint
    from bayesic_amd.svi import GLMReparamSVI
    B, D, S, seed, lr, scale, tau = 5000, 64, 8, 21, 0.02, 7.0, 1.5
    for link, builder in (("logistic", logistic_regression_log_joint), ("poisson", poisson_regression_log_joint)):
        X, y = _regression_data(link, B, D, 2)
        lj, v = builder(scale, tau)
        lam0 = ref.init_lam(D)
        eng = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                        lam0=lam0)
        assert eng.route.startswith("fused") and "glm" in eng.route and eng.route_reason is None, eng.route
        hand = GLMReparamSVI(X, y, link=link, n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau,
                             ctx=ctx, lam0=lam0)
        for _ in range(5):
            assert eng.step() is None
            hand.step()
        ctx.sync()
        # the same kernels on the same draws; scale and tau reach the finish fitted from the symbolic log-joint
        npt.assert_allclose(eng.lam, hand.lam.cpu().numpy(), rtol=1e-9, atol=1e-12)
        npt.assert_allclose(eng.elbo, hand.elbo.item(), rtol=1e-9)
        assert eng.t == 5 and eng.grad.shape == (2 * D,)
        # route="general" never takes it
        general = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr,
                            backend=DeviceBackend(ctx), lam0=lam0, route="general")
        assert general.route == "general"


def test_a_width_the_pass_refuses_falls_back_to_the_general_route_with_the_reason(ctx):
    """D = 6: route='auto' sees the envelope BEFORE the first step and evaluates the model as written -- equal to the
    host backend's evaluation on the same draws -- instead of raising BayesicHipError inside step()."""
    from oracle.einsum_eval import NumpyBackend
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint
    B, D, S = 2000, 6, 8
    X, y = _regression_data("logistic", B, D, 4)
    lj, v = logistic_regression_log_joint(5.0, 1.0)
    latents = [(v["W"], D)]
    eng = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=11, lr=1e-2, backend=DeviceBackend(ctx))
    assert eng.route == "general" and "multiple of 4" in eng.route_reason, (eng.route, eng.route_reason)
    with pytest.raises(ValueError, match="multiple of 4"):
        ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, backend=DeviceBackend(ctx), route="fused")
    eps = eng.draw(0)
    host = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=11, lr=1e-2, backend=NumpyBackend(np.float64),
                     noise=lambda step: eps)
    eng.step()
    host.step()
    npt.assert_allclose(eng.elbo, host.elbo, rtol=1e-5)
    assert np.abs(eng.grad - host.grad).max() <= 2e-4 * np.abs(host.grad).max()
