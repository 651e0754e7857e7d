"""The float64 restatement of the softmax-regression pass (tests/_softmax_ref.py) is right, and the driver's argument
checks that need no GPU.  No test here touches a device."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import _glm_ref as glm
import _softmax_ref as ref


def _inputs(B, D, K, S, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, K, D))).astype(np.float32)
    y = rs.randint(0, K, size=B).astype(np.int32)
    return X, y, W


@pytest.mark.parametrize("K", [2, 3, 7])
def test_gradient_is_the_finite_difference_of_ell(K):
    """G = d ell / d W by central differences, float64, rtol 1e-6 on every entry.  The five-point stencil at step
    1e-3 has truncation ~h^4 / 30 and rounding ~1e-16 ell / h with ell ~ 50: ~1e-11 absolute, so the relative bound
    holds for every entry above 1e-5 (asserted)."""
    B, D, S = 40, 8, 2
    X, y, W = _inputs(B, D, K, S, seed=K)
    y[3] = -1                                              # a skipped row is skipped in both
    X64, W64 = X.astype(np.float64), W.astype(np.float64)

    def ell_of(Wv):
        return ref.data_pass_from_logits(np.einsum("nd,skd->nsk", X64, Wv), X64, y)[0]

    _, G = ref.softmax_data_pass(X, y, W)
    h = 1e-3
    fd = np.zeros_like(G)
    for s in range(S):
        for k in range(K):
            for d in range(D):
                f = []
                for step in (2.0, 1.0, -1.0, -2.0):
                    Wv = W64.copy()
                    Wv[s, k, d] += step * h
                    f.append(ell_of(Wv)[s])
                fd[s, k, d] = (-f[0] + 8.0 * f[1] - 8.0 * f[2] + f[3]) / (12.0 * h)
    assert np.abs(G).min() > 1e-5
    npt.assert_allclose(G, fd, rtol=1e-6)


@pytest.mark.parametrize("K", [2, 5, 16])
def test_class_gradients_sum_to_zero(K):
    X, y, W = _inputs(300, 12, K, 3, seed=10 + K)
    _, G = ref.softmax_data_pass(X, y, W)
    assert np.abs(G.sum(axis=1)).max() <= 1e-12 * np.abs(G).max()


def test_two_classes_are_logistic_regression():
    B, D, S = 500, 16, 4
    X, y, W = _inputs(B, D, 2, S, seed=2)
    W = (np.round(W * 1024.0) / 1024.0).astype(np.float32)     # w1 - w0 is then exact in float32, as the GLM reads it
    ell, G = ref.softmax_data_pass(X, y, W)
    ell_l, G_l = glm.glm_data_pass("logistic", X, y.astype(np.float32), W[:, 1, :] - W[:, 0, :])
    npt.assert_allclose(ell, ell_l, rtol=1e-12)
    npt.assert_allclose(G[:, 1, :], G_l, rtol=1e-12, atol=1e-12 * np.abs(G_l).max())
    npt.assert_allclose(-G[:, 0, :], G_l, rtol=1e-12, atol=1e-12 * np.abs(G_l).max())


def test_extreme_logits_stay_finite():
    """Logits of +-80 and all-equal logits of 80: exp(80) overflows float32, the maximum-subtracted forms do not."""
    K, D = 4, 8
    X = np.eye(D, dtype=np.float32)
    W = np.zeros((2, K, D), np.float32)
    W[0] = 80.0 * (-1.0) ** (np.arange(K)[:, None] + np.arange(D)[None, :])
    W[1] = 80.0
    y = (np.arange(D) % K).astype(np.int32)
    ell, G = ref.softmax_data_pass(X, y, W)
    assert np.isfinite(ell).all() and np.isfinite(G).all()
    npt.assert_allclose(ell[1], -D * math.log(K), rtol=1e-12)        # all classes equal: uniform
    out = ref.predict(X, W, y)
    assert np.isfinite(out["prob"]).all() and np.isfinite(out["lpd"]).all()
    npt.assert_allclose(out["prob"].sum(axis=1), 1.0, rtol=1e-12)


def test_rows_with_labels_outside_the_classes_are_skipped():
    X, y, W = _inputs(60, 8, 3, 2, seed=5)
    y2 = y.copy()
    y2[[4, 17]] = [-1, 3]
    keep = np.ones(60, bool)
    keep[[4, 17]] = False
    a = ref.softmax_data_pass(X, y2, W)
    b = ref.softmax_data_pass(X[keep], y[keep], W)
    npt.assert_allclose(a[0], b[0], rtol=1e-13)
    npt.assert_allclose(a[1], b[1], rtol=1e-13, atol=1e-13)
    p = ref.predict(X, W, y2)
    assert p["lpd"][4] == 0.0 and p["lpd"][17] == 0.0 and (p["lpd"][keep] < 0.0).all()


def test_predictive_of_one_draw_is_its_softmax():
    X, y, W = _inputs(30, 8, 5, 1, seed=6)
    out = ref.predict(X, W, y)
    L = ref.logits(X, W)[:, 0, :]
    npt.assert_allclose(out["prob"], ref.softmax(L), rtol=1e-14)
    npt.assert_allclose(out["lpd"], np.log(ref.softmax(L))[np.arange(30), y], rtol=1e-12)


@pytest.mark.parametrize("K,D,S", [(3, 256, 64), (10, 64, 5)])
def test_float32_evaluation_on_the_cpu_stays_inside_the_device_bounds(K, D, S):
    """The bounds the GPU tests hold the device to (tests/test_softmax_regression_gpu.py's docstring) must hold for a
    plain float32 evaluation of the same formulae on the CPU; a bound that does not is wrong, not the device."""
    B = 400
    X, y, W = _inputs(B, D, K, S, seed=K + D)
    f32 = np.float32
    L = np.einsum("nd,skd->nsk", X, W).astype(f32)
    m = L.max(axis=2, keepdims=True)
    e = np.exp(L - m, dtype=f32)
    s = e.sum(axis=2, keepdims=True, dtype=f32)
    p = (e / s).astype(f32)
    lp = (L[np.arange(B), :, y] - (m[:, :, 0] + np.log(s[:, :, 0], dtype=f32))).astype(f32)
    mx = lp.max(axis=1, keepdims=True)
    lpd = (mx[:, 0] + np.log(np.exp(lp - mx, dtype=f32).sum(axis=1, dtype=f32), dtype=f32) - f32(math.log(S))).astype(f32)
    r, b = ref.predict(X, W, y), ref.predict_bounds(X, W, y)
    assert (np.abs(p.mean(axis=1, dtype=f32) - r["prob"]) <= b["prob"]).all()
    assert (np.abs(lpd - r["lpd"]) <= b["lpd"]).all()
    ell_r, _ = ref.softmax_data_pass(X, y, W)
    assert (np.abs(lp.sum(axis=0, dtype=np.float64) - ell_r) <= 2e-5 * ref.ell_bound(X, y, W)).all()


def test_driver_and_entry_points_are_declared():
    from bayesic_amd import _ffi
    from bayesic_amd.svi import SoftmaxReparamSVI
    import inspect
    names = list(inspect.signature(SoftmaxReparamSVI.__init__).parameters)
    assert names == ["self", "X", "y", "n_classes", "n_total", "n_samples", "seed", "lr", "prior_precision", "ctx",
                     "group", "lam0", "covariance"]
    for member in ("set_batch", "sample", "data_pass", "all_reduce", "step", "params", "covariance", "predict",
                   "heldout_lpd"):
        assert callable(getattr(SoftmaxReparamSVI, member))
    for name in ("bsc_softmax_data_pass", "bsc_softmax_predict_pass"):
        assert name in _ffi.SIGNATURES


def test_driver_argument_errors_come_before_any_device_work():
    """Every check below is made on the host arrays before a context is asked for: no GPU needed."""
    from bayesic_amd.svi import SoftmaxReparamSVI
    X = np.zeros((10, 8), np.float32)
    y = (np.arange(10) % 3).astype(np.int32)
    with pytest.raises(ValueError, match="covariance"):
        SoftmaxReparamSVI(X, y, 3, covariance="lowrank")
    with pytest.raises(ValueError, match="n_classes=1 "):
        SoftmaxReparamSVI(X, y, 1)
    with pytest.raises(ValueError, match="n_classes=17 "):
        SoftmaxReparamSVI(X, y, 17)
    with pytest.raises(ValueError, match="prior_precision"):
        SoftmaxReparamSVI(X, y, 3, prior_precision=0.0)
    with pytest.raises(ValueError, match=r"X must be \[B, D\]"):
        SoftmaxReparamSVI(X, y[:9], 3)
    with pytest.raises(TypeError, match="integer class labels"):
        SoftmaxReparamSVI(X, y.astype(np.float32), 3)
    import torch
    with pytest.raises(TypeError, match="int32"):
        SoftmaxReparamSVI(X, torch.from_numpy(y.astype(np.float32)), 3)
    with pytest.raises(ValueError, match=r"labels in \[0, 2\]; n_classes = 2"):
        SoftmaxReparamSVI(X, y, 2)
    bad = y.copy()
    bad[5] = -1
    with pytest.raises(ValueError, match=r"labels in \[-1, 2\]"):
        SoftmaxReparamSVI(X, bad, 3)
    with pytest.raises(ValueError, match="n_classes \\* D <= 256"):
        SoftmaxReparamSVI(np.zeros((10, 256), np.float32), y, 10, covariance="full")
    with pytest.raises(ValueError, match="multiple of 4"):
        SoftmaxReparamSVI(np.zeros((10, 6), np.float32), y, 3, covariance="full")


def test_family_of_knows_the_new_driver_and_keeps_the_old_answers():
    from bayesic_amd.svi.predict import family_of

    class Glm:
        link = "poisson"

    class Blr:
        family = None

    class Soft:
        link = None
        n_classes = 4

    assert family_of(Glm()) == "poisson" and family_of(Blr()) == "gaussian" and family_of(Soft()) == "softmax"
