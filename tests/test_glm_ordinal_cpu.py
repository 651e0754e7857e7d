"""The float64 restatement of the ordinal route (tests/_glm_ordinal_ref.py) against central differences and against the
direct definition, the pass's float32 forms against that restatement, and the host side of svi/glm_ordinal.py and its
routing in svi/predict.py -- no device.

The device tolerance (tests/test_glm_ordinal_gpu.py) is EPS = 2e-5 times the reference's bound quantities; a plain float32
evaluation of the pass's forms has to stay below EPS / 20 of them here, which leaves a factor 20 for the device's
summation order and its fast logarithm.  Measured at 2000 x 12, S = 8, K = 6: ell 1.4e-8 and G 2.8e-8 of the bound
quantities; the worst over the shapes below is 5.8e-8 (printed)."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import _glm_ordinal_ref as ref

F32_REACH = ref.EPS / 20.0


def _check_inputs(X, y, Z, o, v, K):
    """The conditions make_inputs promises (tests/_glm_ordinal_ref.py)."""
    B, D = X.shape
    keep = np.ones(B, bool) if v is None else v > 0
    assert set(y[keep]) == set(range(K)), "every level occurs among the kept rows"
    W, theta = ref.split(Z, D, K)
    if K > 2:
        assert ref.GAP_LO <= theta[:, 1:].min() and theta[:, 1:].max() <= ref.GAP_HI
    assert np.abs(ref.obs.logits(X, W, o)).max() <= ref.ETA_MAX
    if v is not None:
        assert 0 < (~keep).sum() <= 0.1 * B
        dead = set(y[~keep])
        assert dead >= {-1, K, 2 ** 31 - 1} and not (dead & set(range(K)))


# ---- the reference itself ---------------------------------------------------------------------------------------------------

def test_cutpoints_are_ordered_and_rounded_to_float32():
    theta = np.array([[-0.3, 0.0, -3.0, 1.5], [2.0, -1.0, 0.5, 0.25]], np.float32)
    c = ref.cutpoints(theta)
    assert (np.diff(c, axis=1) > 0).all()
    npt.assert_array_equal(c, c.astype(np.float32).astype(np.float64))
    npt.assert_allclose(c[0], np.cumsum([-0.3, 1.0, math.exp(-3.0), math.exp(1.5)]), rtol=1e-6)
    from bayesic_amd.svi.glm_ordinal import cutpoints
    npt.assert_allclose(cutpoints(theta), c, rtol=1e-6)


def test_log_p_is_the_log_of_the_difference_of_two_sigmoids_and_the_classes_add_up_to_one():
    B, D, S, K = 300, 8, 4, 5
    X, y, Z, o, _ = ref.make_inputs(B, D, S, K, seed=3, mode="offset")
    probs = ref.class_probs(X, Z, K, o)[0]
    npt.assert_allclose(probs.sum(axis=2), 1.0, rtol=0, atol=1e-14)
    t = ref._terms(X, y, Z, K, o, None)
    want = np.log(np.take_along_axis(probs, np.broadcast_to(y[:, None, None], (B, S, 1)).astype(np.int64), axis=2))[:, :, 0]
    npt.assert_allclose(t["raw_logp"], want, rtol=1e-10, atol=1e-12)
    # the product form the pass uses (include/bayesic_hip.h) is the same number: sigma(b) - sigma(a) =
    # sigma(b) sigma(-a) (1 - e^{a - b})
    W, theta = ref.split(Z, D, K)
    c = ref.cutpoints(theta)
    eta = ref.obs.logits(X, W, o)
    worst = 0.0
    for n in range(B):
        k = int(y[n])
        if 0 < k < K - 1:
            a, b = c[:, k - 1] - eta[n], c[:, k] - eta[n]
            form = -ref._sp(-b) - ref._sp(a) + np.log(-np.expm1(-(c[:, k] - c[:, k - 1])))
            worst = max(worst, np.abs(form - t["raw_logp"][n]).max())
    assert worst < 2e-12, worst


@pytest.mark.parametrize("K,mode", [(2, "both"), (3, "offset"), (6, "both"), (8, "weights")])
def test_G_is_the_derivative_of_ell_in_all_P_columns(K, mode):
    """Central differences in float64 over every column of z = [w | theta].  The reference rounds the draws and the
    cutpoints to float32, so the differences are taken on an unrounded twin of its formulas: the same _terms with the
    rounding switched off."""
    B, D, S = 120, 4, 3
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=K, mode=mode)
    _, G = ref.data_pass(X, y, Z, K, o, v)
    P = D + K - 1

    def ell_at(Zp):
        W, th = Zp[:, :D], Zp[:, D:]
        c = np.cumsum(np.concatenate([th[:, :1], np.exp(th[:, 1:])], axis=1), axis=1)
        cpad = np.concatenate([np.full((S, 1), -np.inf), c, np.full((S, 1), np.inf)], axis=1)
        eta = X.astype(np.float64) @ W.T + (0.0 if o is None else o.astype(np.float64)[:, None])
        vv = np.ones(B) if v is None else v.astype(np.float64)
        keep = (vv > 0) & (y >= 0) & (y < K)
        yq = np.where(keep, y, 0).astype(np.int64)
        p = ref._sig(cpad[:, yq + 1].T - eta) - ref._sig(cpad[:, yq].T - eta)
        return (np.where(keep, vv, 0.0)[:, None] * np.where(keep[:, None], np.log(p), 0.0)).sum(axis=0)

    # the cutpoints of the reference are float32-rounded: 6e-8 relative, which moves G by that much -- far below the
    # tolerance of the differences
    Z64 = Z.astype(np.float64)
    h = 1e-5
    for col in range(P):
        Zp, Zm = Z64.copy(), Z64.copy()
        Zp[:, col] += h
        Zm[:, col] -= h
        num = (ell_at(Zp) - ell_at(Zm)) / (2.0 * h)
        npt.assert_allclose(G[:, col], num, rtol=2e-6, atol=2e-6 * np.abs(G).max(), err_msg="column %d" % col)


def test_dropped_rows_add_nothing_whatever_they_hold():
    B, D, S, K = 200, 8, 3, 4
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=9)
    _check_inputs(X, y, Z, o, v, K)
    keep = v > 0
    ell, G = ref.data_pass(X, y, Z, K, o, v)
    ell2, G2 = ref.data_pass(X[keep], y[keep], Z, K, o[keep], v[keep])
    npt.assert_allclose(ell, ell2, rtol=1e-13)
    npt.assert_allclose(G, G2, rtol=1e-12, atol=1e-12)
    # an out-of-range label with a positive weight is dropped too
    y3, v3 = y.copy(), np.where(keep, v, 1.0).astype(np.float32)
    ell3, G3 = ref.data_pass(X, y3, Z, K, o, v3)
    npt.assert_allclose(ell3, ell, rtol=1e-13)
    npt.assert_allclose(G3, G, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,D,S,K,mode", [(2000, 12, 8, 6, "both"), (1003, 12, 3, 2, "none"), (517, 200, 11, 8, "offset"),
                                          (1029, 256, 8, 5, "weights"), (1003, 256, 8, 3, "both")])
def test_plain_float32_stays_inside_the_bounds_at_the_gpu_shapes(B, D, S, K, mode):
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=B + D + S + K, mode=mode)
    _check_inputs(X, y, Z, o, v, K)
    want = ref.data_pass(X, y, Z, K, o, v)
    bnd = ref.bounds(X, y, Z, K, o, v)
    got = ref.data_pass_f32(X, y, Z, K, o, v)
    r_ell, r_G = (float((np.abs(g - w) / (b + 1e-300)).max()) for g, w, b in zip(got, want, bnd))
    print("float32 at B=%d D=%d S=%d K=%d: ell %.3g, G %.3g of the bound quantities (reach %.3g)" % (
        B, D, S, K, r_ell, r_G, F32_REACH))
    assert max(r_ell, r_G) <= F32_REACH


def test_the_predictive_reference_is_consistent():
    B, D, S, K = 150, 8, 6, 5
    X, y, Z, o, _ = ref.make_inputs(B, D, S, K, seed=4, mode="offset")
    y = y.copy()
    y[7], y[8] = -1, K
    out = ref.predict(X, Z, K, y, o)
    npt.assert_allclose(out["prob"].sum(axis=1), 1.0, atol=1e-14)
    assert out["lpd"][7] == 0.0 and out["lpd"][8] == 0.0
    ok = (y >= 0) & (y < K)
    probs = ref.class_probs(X, Z, K, o)[0]
    direct = np.log(probs[np.arange(B), :, np.where(ok, y, 0)].mean(axis=1))
    npt.assert_allclose(out["lpd"][ok], direct[ok], rtol=1e-10)
    npt.assert_allclose(out["lpd_sum"], direct[ok].sum(), rtol=1e-10)
    v = np.linspace(0.0, 2.0, B).astype(np.float32)
    npt.assert_allclose(ref.predict(X, Z, K, y, o, v)["lpd_sum"], (v * out["lpd"]).sum(), rtol=1e-12)


FIT = dict(B=4000, S=8, seed=31, steps=150, lr=0.05)      # tests/test_glm_ordinal_gpu.py runs the device at the same


def test_the_reference_driver_alone_beats_the_class_frequencies_at_the_step_count_of_the_gpu_test():
    """What tests/test_glm_ordinal_gpu.py asks of the device's fit, asked of the float64 reference driver first: the ELBO
    rises from the first step to the last and the held-out log density at the fitted mean beats the training class
    frequencies on fresh rows -- a baseline that comes from the data."""
    K = 5
    X, y = ref.simulate(FIT["B"], 5)
    Xt, yt = ref.simulate(2000, 6)
    assert set(y) == set(range(K))
    lam, elbos = ref.fit(X, y, K, FIT["S"], FIT["seed"], FIT["steps"], FIT["lr"])
    assert elbos[-1] > elbos[0]
    P = X.shape[1] + K - 1
    Z = ref.posterior_draws(lam, P, 64, FIT["seed"])
    score = ref.predict(Xt, Z, K, yt)["lpd_sum"] / len(yt)
    base = ref.frequency_baseline(y, yt, K)
    print("reference fit: ELBO %.1f -> %.1f, held-out lpd %.4f against the class frequencies' %.4f; cutpoints %s" % (
        elbos[0], elbos[-1], score, base, ref.cutpoints(lam[None, X.shape[1]:P])[0]))
    assert score > base + 0.1


# ---- the driver's host side ---------------------------------------------------------------------------------------------

class FakeCtx:
    """A context without a device: host tensors, every C-ABI call recorded and not made."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def info(self):
        return {"cu_count": 256}

    def reserve(self, n):
        self.reserved = n

    def to_device(self, a, dtype=None):
        import torch
        t = torch.as_tensor(np.ascontiguousarray(a))
        return t if dtype is None else t.to(dtype)

    def call(self, name, *a):
        self.calls.append((name, a))


def _data(B=40, D=4, K=5, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal((B, D)).astype(np.float32), (np.arange(B) % K).astype(np.int32)


def test_constructor_refusals_and_messages():
    from bayesic_amd.svi import OrdinalReparamSVI
    X, y = _data()
    ctx = FakeCtx()
    for K in (1, 9):
        with pytest.raises(ValueError, match=r"n_levels=%d must be in \[2, 8\]" % K):
            OrdinalReparamSVI(X, y, K, ctx=ctx)
    with pytest.raises(ValueError, match=r"y has labels in \[0, 4\]; n_classes = 4 needs them in \[0, 4\)"):
        OrdinalReparamSVI(X, y, 4, ctx=ctx)
    with pytest.raises(ValueError, match="labels in \\[-1, 4\\]"):
        OrdinalReparamSVI(X, np.where(y == 2, -1, y).astype(np.int32), 5, ctx=ctx)
    with pytest.raises(TypeError, match="integer class labels"):
        OrdinalReparamSVI(X, y.astype(np.float32), 5, ctx=ctx)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        OrdinalReparamSVI(X, y, 5, prior_precision=0.0, ctx=ctx)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        OrdinalReparamSVI(X, y, 5, n_samples=65, ctx=ctx)
    with pytest.raises(ValueError, match="covariance must be 'diag' or 'full'"):
        OrdinalReparamSVI(X, y, 5, covariance="lowrank", ctx=ctx)
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| theta \(4\)\] needs 16"):
        OrdinalReparamSVI(X, y, 5, lam0=np.zeros(8), ctx=ctx)
    with pytest.raises(ValueError, match=r"X must be \[B, D\] and y \[B\]"):
        OrdinalReparamSVI(X, y[:-1], 5, ctx=ctx)
    with pytest.raises(ValueError, match="weights must be finite and >= 0"):
        OrdinalReparamSVI(X, y, 5, weights=-np.ones(40, np.float32), ctx=ctx)
    with pytest.raises(TypeError):
        OrdinalReparamSVI(X, y, 5, exposure=np.ones(40, np.float32), ctx=ctx)      # there is no exposure keyword
    assert not ctx.calls


def test_full_covariance_is_accepted_at_five_levels_and_refused_at_four():
    from bayesic_amd.svi import OrdinalReparamSVI
    X, y = _data()
    m = OrdinalReparamSVI(X, y, 5, covariance="full", ctx=FakeCtx())
    assert m.P == 8 and m.lam.numel() == 8 + 8 * 9 // 2
    with pytest.raises(ValueError, match=r"covariance='full' needs D \+ n_levels - 1 <= 256 and a multiple of 4 "
                                         r"\(bsc_glm_fullrank_update\); got 4 \+ 4 - 1 = 7"):
        OrdinalReparamSVI(X, (y % 4).astype(np.int32), 4, covariance="full", ctx=FakeCtx())
    Xw = np.zeros((40, 256), np.float32)
    with pytest.raises(ValueError, match=r"got 256 \+ 5 - 1 = 260"):
        OrdinalReparamSVI(Xw, y, 5, covariance="full", ctx=FakeCtx())


def test_the_model_is_routed_as_ordinal_and_the_family_lists_are_untouched():
    from bayesic_amd.svi import OrdinalReparamSVI
    from bayesic_amd.svi import predict as mod
    X, y = _data()
    m = OrdinalReparamSVI(X, y, 5, ctx=FakeCtx())
    assert not hasattr(m, "n_classes") and m.n_levels == m.K == 5 and m.link == "ordinal"
    assert mod.family_of(m) == "ordinal"
    assert mod.family_of(OrdinalReparamSVI.__new__(OrdinalReparamSVI)) == "ordinal"
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}
    # the default start is ordered with unit gaps
    npt.assert_array_equal(m.params()["cutpoints"], np.arange(4.0))
    npt.assert_array_equal(m.params()["theta"][0], np.zeros(4))
    assert m.params()["w"][0].shape == (4,) and m.covariance().shape == (8, 8)


@pytest.mark.parametrize("covariance,finish", [("diag", "bsc_glm_update"), ("full", "bsc_glm_fullrank_update")])
def test_three_steps_are_noise_then_pass_and_finish_three_times(covariance, finish):
    import torch
    from bayesic_amd.svi import OrdinalReparamSVI
    X, y = _data()
    o, v = np.ones(40, np.float32), np.ones(40, np.float32)
    ctx = FakeCtx()
    m = OrdinalReparamSVI(X, y, 5, n_samples=3, covariance=covariance, ctx=ctx, offset=o, weights=v)
    for _ in range(3):
        m.step()
    names = [c[0] for c in ctx.calls]
    assert names == ["bsc_blr_noise"] + ["bsc_glm_ordinal_data_pass", finish] * 3
    name, a = ctx.calls[1]
    # (X, ldx, y, offset, weight, B, D, K, Z, ldz, S, ell, G): the draws are the driver's W, [S, P] contiguous
    assert a[0] is m.X and a[1] == 4 and a[2] is m.y and a[3] is m.offset and a[4] is m.weights
    assert a[5:8] == (40, 4, 5) and a[9] == 8 and a[10] == 3
    assert a[8].numel() == 3 * 8 and a[8].dtype == torch.float32
    assert a[11].numel() == 3 and a[12].numel() == 3 * 8
    assert ctx.calls[2][1][7:9] == (8, 3)                      # the finish at D := P
    assert ctx.calls[3][1][8].data_ptr() != a[8].data_ptr()      # the double buffer flipped
    # set_batch: labels are range-checked with tensors, raw pointers are taken as they are; None drops the vectors
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    with pytest.raises(ValueError, match="labels in \\[1, 5\\]"):
        m.set_batch(Xt, yt + 1)
    with pytest.raises(TypeError, match="y must be int32"):
        m.set_batch(Xt, yt.to(torch.int64))
    m.set_batch(Xt, yt)
    assert m.offset is None and m.weights is None and m._oarg is None
    m.set_batch(1234, 5678, rows=7, offset=91, weights=92)
    assert (m._Xarg, m._yarg, m.B, m._oarg, m._varg, m.y) == (1234, 5678, 7, 91, 92, None)


def test_predict_routes_through_the_models_own_pass():
    import torch
    from bayesic_amd.svi import OrdinalReparamSVI
    from bayesic_amd.svi import predict as mod
    X, y = _data()
    ctx = FakeCtx()
    m = OrdinalReparamSVI(X, y, 5, ctx=ctx, offset=np.zeros(40, np.float32))
    Z = torch.zeros((6, 8), dtype=torch.float32)
    with pytest.raises(ValueError, match="fitted with an offset"):
        mod.predict(m, X, y, draws=(Z, None))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, draws=(Z, None), groups=np.zeros(40, np.int32))
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not ordinal"):
        mod.predict(m, X, y, draws=(Z, None), upper=np.zeros(40, np.float32))
    with pytest.raises(ValueError, match=r"draws of the ordinal model are \(Z float32 \[S, 8\], None\)"):
        m.predict(X, y, draws=(torch.zeros((6, 4)), None), offset=np.zeros(40, np.float32))
    out = mod.predict(m, X, y, draws=(Z, None), offset=np.zeros(40, np.float32))
    name, a = ctx.calls[-1]
    assert name == "bsc_ordinal_predict_pass" and a[4:7] == (40, 4, 5) and a[7] is Z and a[8:10] == (8, 6)
    assert set(out) == {"prob", "lpd", "lpd_sum"} and tuple(out["prob"].shape) == (40, 5)
    out = m.predict(X, draws=(Z, None), offset=np.zeros(40, np.float32))
    assert set(out) == {"prob"} and ctx.calls[-1][1][2] is None
    out = m.predict(X, y, draws=(Z, None), offset=np.zeros(40, np.float32), weights=np.ones(40, np.float32))
    assert set(out) == {"prob", "lpd", "lpd_sum", "weight_sum"} and float(out["weight_sum"]) == 40.0
    # posterior_draws: width P on Philox stream 2
    draws = mod.posterior_draws(m, 6)
    name, a = ctx.calls[-1]
    assert name == "bsc_philox_normal" and a[1] == mod.PREDICT_STREAM and a[3:5] == (6, 8)
    assert draws[1] is None and tuple(draws[0].shape) == (6, 8) and draws[0].dtype == torch.float32
