"""GPU parity of the softmax-regression path (csrc/bsc_softmax.hip through the C ABI, svi/softmax.py) against the
float64 restatement in tests/_softmax_ref.py.

Tolerances (the project's existing ones for this arithmetic: a float32 dot of <= 256 terms, transcendentals, float64
finish):
 * ell: |dev - ref| <= 2e-5 * sum_n (|l[n,s,y_n]| + |lse[n,s]| + 1)   (test_glm_gpu's bound, the two terms of a row);
 * G: rtol 1e-4, atol 1e-4 * max|G|                                   (test_glm_gpu);
 * the finish from given statistics (float64 both sides): rtol 1e-9   (test_glm_gpu);
 * whole updates against the reference: ELBO rtol 1e-6, gradient 1e-4 * max|grad|, lam atol 2e-4 (test_glm_gpu);
 * the full guide: ELBO rtol 1e-6, lam atol 1e-4                      (test_glm_full_gpu's driver test).
Predictive bounds (test_predict_gpu's idiom): with a = max_k sum_d |x_nd w_skd| the logit of a draw is off by at most
2e-5 (a + 1).  softmax_k has derivative p_k (1[j = k] - p_j) in logit j, so |d p_k| <= 2 p_k max_j |d l_j|, and the
exponential, sum and quotient add a relative 2e-5 at most:
    |prob - ref|   <= mean_s 2e-5 (2 p_nsk a + p_nsk)
    |lpd_n - ref|  <= max_s 2 * 2e-5 (a + |lse| + 1)    (l_y and lse each carry the logit error; log-mean-exp is a
                                                         contraction in the sup norm)
    lpd_sum within the sum of those.
tests/test_softmax_cpu.py holds the float32 CPU evaluation of the reference inside these bounds."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_full_ref as fr
import _glm_ref as glm
import _softmax_ref as ref

pytestmark = pytest.mark.gpu

KS = (2, 3, 5, 8, 10, 16)


def _pass(ctx, X, y, W, ld=None, y_offset=False):
    """bsc_softmax_data_pass on host arrays; ``ld``: X sits in a wider buffer of that leading dimension whose padding
    is 7.0; ``y_offset``: y starts 4 bytes into its buffer."""
    B, D = X.shape
    S, K = W.shape[:2]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    if y_offset:
        yd = ctx.to_device(np.concatenate([[1], y]).astype(np.int32))[1:]
    else:
        yd = ctx.to_device(np.asarray(y, np.int32))
    Wd = ctx.to_device(W)
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, K, D), torch.float64)
    ctx.call("bsc_softmax_data_pass", Xd, (ld or D), yd, B, D, K, Wd, S, ell, G)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy()


def _inputs(B, D, K, S, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, K, D))).astype(np.float32)
    y = rs.randint(0, K, size=B).astype(np.int32)
    return X, y, W


def _assert_pass(ell, G, X, y, W, tag=""):
    ell_r, G_r = ref.softmax_data_pass(X, y, W)
    bound = ref.ell_bound(X, y, W)
    err = np.abs(ell - ell_r)
    gmax = np.abs(G_r).max() if G_r.size else 0.0
    print("%s B=%d D=%d K=%d S=%d: ell err/bound %.3g, G err/max %.3g" % (
        tag, X.shape[0], X.shape[1], W.shape[1], W.shape[0], (err / (bound + 1e-300)).max(),
        np.abs(G - G_r).max() / (gmax + 1e-300)))
    assert (err <= 2e-5 * bound + 1e-12).all(), (err / (bound + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * gmax)
    return ell_r, G_r


def _draw_counts(K):
    g = 16 // K
    return sorted({1, g, g + 1, 2 * g + 1} | ({64} if K == 16 else set()))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("D", [256, 252, 64, 4])
@pytest.mark.parametrize("B", [0, 5, 16, 17, 1003])
def test_pass_matches_the_reference(ctx, B, D, K):
    for S in _draw_counts(K):        # straddles the draws-per-launch g = floor(16 / K)
        X, y, W = _inputs(B, D, K, S, seed=B * 7 + D + 31 * K + S)
        ell, G = _pass(ctx, X, y, W)
        _assert_pass(ell, G, X, y, W)
        if B == 0:
            assert (ell == 0).all() and (G == 0).all()


@pytest.mark.parametrize("K", KS)
def test_pass_with_more_than_one_tile_per_wave(ctx, K):
    """B = 33 000 > 2 048 resident waves x 16 rows: every wave runs a second tile.  The row count assumes 256 CUs (an
    MI355X); on a larger device this is one tile per wave again.  tests/test_regression_multi_tile_gpu.py sizes its
    batches from the device's CU count and goes on to three tiles per wave."""
    S = 16 // K + 1
    X, y, W = _inputs(33000, 256, K, S, seed=K)
    ell, G = _pass(ctx, X, y, W)
    _assert_pass(ell, G, X, y, W)


@pytest.mark.parametrize("B,D,ld", [(333, 64, 96), (1003, 256, 260)])
@pytest.mark.parametrize("K", [3, 16])
def test_pass_respects_the_leading_dimension(ctx, B, D, ld, K):
    X, y, W = _inputs(B, D, K, 16 // K + 1, seed=ld + K)
    ell, G = _pass(ctx, X, y, W, ld=ld)
    _assert_pass(ell, G, X, y, W)


def test_pass_with_a_y_that_is_not_16_byte_aligned(ctx):
    """D = 256 with y starting 4 bytes into its buffer: the same kernel (y is loaded 4 bytes at a time)."""
    X, y, W = _inputs(1003, 256, 5, 4, seed=3)
    ell, G = _pass(ctx, X, y, W, y_offset=True)
    _assert_pass(ell, G, X, y, W)


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("K", [3, 16])
def test_operand_layout_with_exact_integers(ctx, K, D):
    """One-hot rows (row n has a single 1 in column 3 n mod D), integer weights W[s, k, d] in {-3 .. 3} that depend on
    the draw, the class and the column, labels n mod K: every logit is a small integer, l[n, s, k] = W[s, k, 3 n mod D],
    and any mix-up of the row, draw, class or column mapping changes ell or G by O(1).  S = g + 1 takes two launches.
    The bounds: the logits are exact, expf / logf are good to an ulp and the K-term sum adds (K - 1) roundings, so a
    probability carries (K + 3) 2^-24 <= 1.2e-6 relative (G: rtol 2e-6, atol 2e-7 for 1 - p formed at ulp(1)) and a
    row's log-probability 2e-6 absolute (ell: B * 2e-6)."""
    B, S = (96, 16 // K + 1) if D == 256 else (40, 16 // K + 1)
    n = np.arange(B)
    X = np.zeros((B, D), np.float32)
    X[n, (3 * n) % D] = 1.0
    s_, k_, d_ = np.meshgrid(np.arange(S), np.arange(K), np.arange(D), indexing="ij")
    W = (((3 * s_ + 5 * k_ + 7 * (d_ % 11) + (s_ * k_) % 3 + (s_ * d_) % 5) % 7) - 3).astype(np.float32)
    y = (n % K).astype(np.int32)
    ell, G = _pass(ctx, X, y, W)
    ell_r, G_r = ref.softmax_data_pass(X, y, W)
    npt.assert_allclose(ell, ell_r, rtol=0, atol=B * 2e-6)
    npt.assert_allclose(G, G_r, rtol=2e-6, atol=2e-7)
    assert len(set(np.round(ell_r, 3))) == S and len(set(np.round(G_r.ravel(), 4))) > 8
    L = ref.logits(X, W)
    assert (L == np.round(L)).all() and len(np.unique(L)) == 7


@pytest.mark.parametrize("B,D", [(1003, 256), (333, 64)])
def test_two_classes_against_the_shipped_logistic_kernel(ctx, B, D):
    """K = 2 with W = [0, w] is logistic regression with weights w: bsc_glm_data_pass on the same data.  Both sides
    are within their own bound of float64, so they differ by the sum of the two at most."""
    S = 9
    X, y, W = _inputs(B, D, 2, S, seed=B)
    W[:, 0, :] = 0.0
    ell, G = _pass(ctx, X, y, W)
    yf = y.astype(np.float32)
    w = np.ascontiguousarray(W[:, 1, :])
    ell_l, G_l = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    ctx.call("bsc_glm_data_pass", 0, ctx.to_device(X), D, ctx.to_device(yf), B, D, ctx.to_device(w), S, ell_l, G_l)
    ctx.sync()
    ell_l, G_l = ell_l.cpu().numpy(), G_l.cpu().numpy()
    L = X.astype(np.float64) @ w.astype(np.float64).T
    A, _ = glm.log_partition("logistic", L)
    bound = 2e-5 * (ref.ell_bound(X, y, W) + (np.abs(yf.astype(np.float64)[:, None] * L) + A + 1.0).sum(axis=0))
    print("ell diff/bound %.3g" % (np.abs(ell - ell_l) / bound).max())
    assert (np.abs(ell - ell_l) <= bound).all()
    gmax = np.abs(G_l).max()
    npt.assert_allclose(G[:, 1, :], G_l, rtol=2e-4, atol=2e-4 * gmax)
    npt.assert_allclose(-G[:, 0, :], G_l, rtol=2e-4, atol=2e-4 * gmax)


@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
def test_extreme_logits(ctx, D, B):
    """Draw 0: logits +-80 alternating over classes and columns; draw 1: every class at +80 (the uniform softmax)."""
    K = 4
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    W = np.zeros((2, K, D), np.float32)
    W[0] = 80.0 * (-1.0) ** (np.arange(K)[:, None] + np.arange(D)[None, :])
    W[1] = 80.0
    y = (np.arange(B) % K).astype(np.int32)
    ell, G = _pass(ctx, X, y, W)
    assert np.isfinite(ell).all() and np.isfinite(G).all()
    assert set(np.unique(ref.logits(X, W))) == {-80.0, 80.0}
    _assert_pass(ell, G, X, y, W)


def test_rows_with_labels_outside_the_classes_change_nothing(ctx):
    K, D, S = 5, 64, 4
    X, y, W = _inputs(1003, D, K, S, seed=8)
    y2 = y.copy()
    skip = np.arange(0, 1003, 7)
    y2[skip] = np.where(np.arange(skip.size) % 2 == 0, -1, K)
    keep = np.ones(1003, bool)
    keep[skip] = False
    ell, G = _pass(ctx, X, y2, W)
    _assert_pass(ell, G, X[keep], y[keep], W, tag="rows removed")
    wild = y.copy()                                   # any int32 is memory-safe: only compared with class indices
    wild[skip] = np.where(np.arange(skip.size) % 2 == 0, np.iinfo(np.int32).min, np.iinfo(np.int32).max)
    ell2, G2 = _pass(ctx, X, wild, W)
    npt.assert_array_equal(ell2, ell)
    npt.assert_array_equal(G2, G)


def test_pass_is_deterministic(ctx):
    X, y, W = _inputs(5000, 256, 3, 11, seed=5)
    a = _pass(ctx, X, y, W)
    b = _pass(ctx, X, y, W)
    npt.assert_array_equal(a[0], b[0])
    npt.assert_array_equal(a[1], b[1])


def test_refusals_name_the_quantity_and_leave_the_outputs(ctx):
    from bayesic_amd._ffi import BayesicHipError
    X, W = ctx.zeros((9, 260)), ctx.zeros(65 * 17 * 8 + 4)
    y = ctx.zeros(9, torch.int32)
    ell = ctx.to_device(np.full(65, -5.0), torch.float64)
    G = ctx.to_device(np.full(65 * 16 * 8, -5.0), torch.float64)
    prob = ctx.to_device(np.full(9 * 16, -5.0, np.float32))
    lpd = ctx.to_device(np.full(9, -5.0, np.float32))

    def call(K=3, D=8, S=8, Wa=W, Ga=G):
        ctx.call("bsc_softmax_data_pass", X, 260, y, 9, D, K, Wa, S, ell, Ga)

    def pcall(K=3, D=8, S=8, Wa=W, ya=y, outs=(prob, lpd, None)):
        ctx.call("bsc_softmax_predict_pass", X, 260, ya, 9, D, K, Wa, S, *outs)

    for f in (call, pcall):
        with pytest.raises(BayesicHipError, match="K=1 must be in"):
            f(K=1)
        with pytest.raises(BayesicHipError, match="K=17 must be in"):
            f(K=17)
        with pytest.raises(BayesicHipError, match="D=6 must be a multiple of 4"):
            f(D=6)
        with pytest.raises(BayesicHipError, match="S=65"):
            f(S=65)
        with pytest.raises(BayesicHipError, match="16-byte aligned"):
            f(Wa=W[1:])
    with pytest.raises(BayesicHipError, match="null output"):
        call(Ga=None)
    with pytest.raises(BayesicHipError, match="need y"):
        pcall(ya=None)
    with pytest.raises(BayesicHipError, match="no output requested"):
        pcall(outs=(None, None, None))
    ctx.sync()
    for out in (ell, G, prob, lpd):
        assert (out.cpu().numpy() == -5.0).all()


@pytest.mark.parametrize("K,D,S", [(3, 8, 5), (10, 256, 3)])
def test_finish_reused_at_K_times_D_parameters(ctx, K, D, S):
    """bsc_glm_update(stats) with D := K D (2 560 at the larger shape): float64 on both sides."""
    P = K * D
    rs = np.random.RandomState(P + S)
    f64 = torch.float64
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    m1, m2 = 0.01 * rs.standard_normal(2 * P), 1e-4 * rs.uniform(size=2 * P)
    ell, G = -100.0 * rs.uniform(1, 2, S), rs.standard_normal((S, P)) * 5
    seed, t, scale, tau, lr = 99, 4, 12.5, 0.7, 0.02
    eps = np.zeros((S, P + 1))
    eps[:, :P] = glm.noise(P, S, seed, t - 1)
    W = glm.draw(lam, eps[:, :P])
    eps_n = np.zeros((S, P + 1))
    eps_n[:, :P] = glm.noise(P, S, seed, t)
    d = dict(stats=ctx.to_device(np.concatenate([ell, G.ravel()]), f64), lam=ctx.to_device(lam, f64),
             out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64), m2=ctx.to_device(m2, f64),
             eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()), eps_n=ctx.to_device(eps_n.ravel(), f64),
             W_n=ctx.zeros(S * P), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64))
    ctx.call("bsc_glm_update", d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], P, S, scale, tau, t,
             lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["elbo"], d["grad"])
    ctx.sync()
    lam_r, m1_r, m2_r, elbo_r, grad_r = glm.finish(lam, m1, m2, t, eps[:, :P], W, ell, G, scale, tau, lr)
    npt.assert_allclose(d["elbo"].item(), elbo_r, rtol=1e-9)
    npt.assert_allclose(d["grad"].cpu().numpy(), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
    npt.assert_allclose(d["out"].cpu().numpy(), lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(d["m1"].cpu().numpy(), m1_r, rtol=1e-9, atol=1e-15)
    npt.assert_allclose(d["m2"].cpu().numpy(), m2_r, rtol=1e-9, atol=1e-18)
    npt.assert_allclose(d["W_n"].cpu().numpy().reshape(S, P), glm.draw(lam_r, eps_n[:, :P]), rtol=2e-7, atol=1e-9)


def _class_data(B, D, K, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    L = X.astype(np.float64) @ (2.0 * rs.standard_normal((K, D))).T
    y = (rs.uniform(size=B)[:, None] > np.cumsum(ref.softmax(L), axis=1)).sum(axis=1).clip(0, K - 1)
    return X, y.astype(np.int32)


@pytest.mark.parametrize("B,D,K,S", [(1003, 64, 5, 8), (2000, 256, 10, 3)])
def test_five_updates_track_the_reference(ctx, B, D, K, S):
    from bayesic_amd.svi import SoftmaxReparamSVI
    seed, lr, tau = 1234, 0.01, 2.0
    X, y = _class_data(B, D, K, seed=B + K)
    model = SoftmaxReparamSVI(X, y, K, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau, ctx=ctx)
    lam = ref.init_lam(K, D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 6):
        assert model.step() is None
        lam, m1, m2, elbo, grad = ref.softmax_step(lam, m1, m2, t, X, y, K, S, seed, 10.0 * B, lr, tau)
        ctx.sync()
        g = model.grad.cpu().numpy()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    p = model.params()
    assert p["m"].shape == (K, D) and p["rho"].shape == (K, D)
    npt.assert_allclose(np.concatenate([p["m"].ravel(), p["rho"].ravel()]), lam, atol=2e-4)
    npt.assert_allclose(model.covariance(), np.diag(np.exp(2.0 * lam[K * D:])), rtol=1e-3)


def test_driver_checks_labels_on_the_device_and_is_deterministic(ctx):
    from bayesic_amd.svi import SoftmaxReparamSVI
    X, y = _class_data(777, 64, 3, seed=1)
    Xd, yd = ctx.to_device(X), ctx.to_device(y)
    bad = yd.clone()
    bad[5] = 3
    with pytest.raises(ValueError, match=r"labels in \[0, 3\]"):
        SoftmaxReparamSVI(Xd, bad, 3, ctx=ctx)
    with pytest.raises(TypeError, match="int32"):
        SoftmaxReparamSVI(Xd, yd.to(torch.float32), 3, ctx=ctx)
    out = []
    for _ in range(2):
        model = SoftmaxReparamSVI(Xd, yd, 3, n_total=7770, n_samples=8, seed=7, lr=0.02, ctx=ctx)
        with pytest.raises(ValueError, match=r"labels in \[0, 3\]"):
            model.set_batch(Xd, bad)
        model.set_batch(Xd, yd)
        for _ in range(4):
            model.step()
        ctx.sync()
        out.append((model.lam.cpu().numpy().copy(), model.elbo.item()))
    npt.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


def test_full_covariance_guide_at_24_parameters(ctx):
    """covariance='full' at (K, D) = (3, 8): bsc_glm_fullrank_update with D := 24, three updates against
    tests/_glm_full_ref.py at that file's driver tolerances; (10, 256) is outside that entry point's envelope."""
    from bayesic_amd.svi import SoftmaxReparamSVI
    K, D, S, B, seed, lr, tau = 3, 8, 8, 500, 11, 0.02, 1.5
    P = K * D
    X, y = _class_data(B, D, K, seed=4)
    model = SoftmaxReparamSVI(X, y, K, n_total=4.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau, ctx=ctx,
                              covariance="full")
    lam = fr.init_lam(P)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 4):
        model.step()
        eps = fr.noise(P, S, seed, t - 1)
        W = fr.draw(lam, eps)
        ell, G = ref.softmax_data_pass(X, y, W.reshape(S, K, D))
        lam, m1, m2, elbo, grad = fr.finish(lam, m1, m2, t, eps, W, ell, G.reshape(S, P), 4.0, tau, lr)
        ctx.sync()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=1e-4)
    p = model.params()
    assert p["m"].shape == (K, D) and p["L"].shape == (P, P) and p["rho"].shape == (K, D)
    npt.assert_allclose(model.covariance(), p["L"] @ p["L"].T, rtol=1e-14)
    with pytest.raises(ValueError, match="n_classes \\* D <= 256"):
        SoftmaxReparamSVI(np.zeros((8, 256), np.float32), np.zeros(8, np.int32), 10, ctx=ctx, covariance="full")


# ---- the predictive ---------------------------------------------------------------------------------------------

def _predict(ctx, X, W, y=None, want=("prob", "lpd", "lpd_sum"), sentinel=-7.0):
    """bsc_softmax_predict_pass on host arrays; outputs not in ``want`` are passed as NULL."""
    B, D = X.shape
    S, K = W.shape[:2]
    bufs = dict(prob=ctx.to_device(np.full((B, K), sentinel, np.float32)),
                lpd=ctx.to_device(np.full(B, sentinel, np.float32)),
                lpd_sum=ctx.to_device(np.full(1, sentinel), torch.float64))
    yd = None if y is None else ctx.to_device(np.asarray(y, np.int32))
    ctx.call("bsc_softmax_predict_pass", ctx.to_device(X), D, yd, B, D, K, ctx.to_device(W), S,
             *[bufs[k] if k in want else None for k in ("prob", "lpd", "lpd_sum")])
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


@pytest.mark.parametrize("S", [1, 64])
@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("K", [3, 10])
@pytest.mark.parametrize("B", [0, 5, 1003])
def test_predictive_matches_the_reference(ctx, B, K, D, S):
    X, y, W = _inputs(B, D, K, S, seed=B + D + K + S)
    if B:
        y[::9] = -1 if K == 3 else K                  # rows with a label outside the classes score 0
    out = _predict(ctx, X, W, y)
    if B == 0:
        assert out["lpd_sum"][0] == 0.0
        return
    r, b = ref.predict(X, W, y), ref.predict_bounds(X, W, y)
    print("B=%d K=%d D=%d S=%d: prob err/bound %.3g, lpd err/bound %.3g" % (
        B, K, D, S, (np.abs(out["prob"] - r["prob"]) / b["prob"]).max(),
        (np.abs(out["lpd"] - r["lpd"]) / (b["lpd"] + 1e-300)).max()))
    assert (np.abs(out["prob"] - r["prob"]) <= b["prob"]).all()
    assert (np.abs(out["lpd"] - r["lpd"]) <= b["lpd"]).all()
    assert (out["lpd"][::9] == 0.0).all()
    assert abs(out["lpd_sum"][0] - r["lpd_sum"]) <= b["lpd_sum"]
    assert np.abs(out["prob"].astype(np.float64).sum(axis=1) - 1.0).max() <= K * 1e-6


def test_predictive_honours_null_outputs_and_is_deterministic(ctx):
    X, y, W = _inputs(333, 64, 5, 7, seed=12)
    full = _predict(ctx, X, W, y)
    for want in (("prob",), ("lpd",), ("lpd_sum",), ("prob", "lpd_sum")):
        out = _predict(ctx, X, W, y, want=want)
        for k in ("prob", "lpd", "lpd_sum"):
            if k in want:
                npt.assert_array_equal(out[k], full[k])
            else:
                assert (out[k] == -7.0).all(), k
    only_prob = _predict(ctx, X, W, None, want=("prob",))
    npt.assert_array_equal(only_prob["prob"], full["prob"])


def test_driver_predict_draws_on_stream_two(ctx):
    from bayesic_amd.svi import SoftmaxReparamSVI, posterior_draws
    from bayesic_amd.svi.predict import family_of
    K, D = 4, 64
    X, y = _class_data(600, D, K, seed=9)
    model = SoftmaxReparamSVI(X[:500], y[:500], K, n_samples=8, seed=21, lr=0.05, ctx=ctx)
    for _ in range(3):
        model.step()
    ctx.sync()
    assert family_of(model) == "softmax"
    W, lv = posterior_draws(model, 16, seed=5)
    assert lv is None and tuple(W.shape) == (16, K, D)
    W_r = ref.posterior_draws(model.lam.cpu().numpy(), K, D, 16, 5)
    npt.assert_allclose(W.cpu().numpy(), W_r, rtol=2e-7, atol=1e-9)
    out = model.predict(X[500:], y[500:], n_samples=16, seed=5)
    r, b = ref.predict(X[500:], W.cpu().numpy(), y[500:]), ref.predict_bounds(X[500:], W.cpu().numpy(), y[500:])
    assert (np.abs(out["prob"].cpu().numpy() - r["prob"]) <= b["prob"]).all()
    assert (np.abs(out["lpd"].cpu().numpy() - r["lpd"]) <= b["lpd"]).all()
    npt.assert_allclose(model.heldout_lpd(X[500:], y[500:], n_samples=16, seed=5), r["lpd_sum"] / 100.0,
                        atol=b["lpd_sum"] / 100.0)
    assert "lpd" not in model.predict(X[500:], n_samples=16, seed=5)
    with pytest.raises(TypeError, match="integer class labels"):
        model.predict(X[500:], y[500:].astype(np.float32))


def test_end_to_end_heldout_score(ctx):
    """K = 3, D = 8, AR(0.9) design (ref.ar_design(4000, 8, 3, seed=7): 3 000 training rows, 1 000 held out), 300
    full-batch updates at lr 0.05, S = 8, 64 predictive draws.

    Recorded from the float64 reference of the same run (tests/_softmax_ref.py on the CPU) BEFORE the device ran:
        held-out lpd per row at t = 0 (seed 1234)     -1.089705
        held-out lpd per row, fitted (seed 1234)      -0.463789
        uniform baseline -log 3                       -1.098612
        class-frequency baseline (training freq.)     -1.085841     (frequencies 0.301, 0.297, 0.402)
        fitted value over Philox seeds 1234, 1, 2, 3, 4:  -0.463789 -0.464965 -0.463085 -0.464207 -0.463362
                                                      mean -0.463882, standard deviation 0.000740
    The device run must beat both baselines and land within three of those standard deviations of the reference's
    fitted value for its seed."""
    from bayesic_amd.svi import SoftmaxReparamSVI
    K, D, S, seed = 3, 8, 8, 1234
    X, y = ref.ar_design(4000, D, K, seed=7)
    Xt, yt, Xh, yh = X[:3000], y[:3000], X[3000:], y[3000:]
    freq = np.bincount(yt, minlength=K) / 3000.0
    base_uniform, base_freq = -math.log(3.0), float(np.log(freq)[yh].mean())
    npt.assert_allclose(base_freq, -1.085841, atol=1e-6)             # the data are the recorded run's
    model = SoftmaxReparamSVI(Xt, yt, K, n_samples=S, seed=seed, lr=0.05, ctx=ctx)
    Xh_d, yh_d = ctx.to_device(Xh), ctx.to_device(yh)
    lpd0 = model.heldout_lpd(Xh_d, yh_d, n_samples=64)
    for _ in range(300):
        model.step()
    lpd = model.heldout_lpd(Xh_d, yh_d, n_samples=64)
    print("held-out lpd per row: t=0 %.6f, fitted %.6f (reference -1.089705, -0.463789)" % (lpd0, lpd))
    assert lpd > base_uniform and lpd > base_freq
    assert abs(lpd - (-0.463789)) <= 3.0 * 0.000740
    assert abs(lpd0 - (-1.089705)) <= 3.0 * 0.000740
