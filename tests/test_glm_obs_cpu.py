"""Offsets, exposure and row weights of the GLM route on the CPU: the float64 reference (tests/_glm_obs_ref.py) against
finite differences, against tests/_glm_ref.py and against the binomial identity; a naive float32 evaluation against the
bounds the device is held to (tests/test_glm_obs_gpu.py); the drivers' argument errors, raised before any device call;
the new entry points in the header and the binding."""
import math
import types

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_obs_ref as ref
import _glm_ref as glm

LINKS = ("logistic", "poisson")


def _inputs(link, B, D, S, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if link == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, W, o)).max()
        if peak > 3.5:
            W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    return X, y, W, o, v


@pytest.mark.parametrize("link", LINKS)
def test_reference_gradient_is_the_derivative_of_its_ell(link):
    """G[s] = d ell[s] / d w_s by central differences (float64 weights, so the reference's float32 rounding of W is the
    identity: the perturbed weights are kept exactly representable steps apart only in float64, hence the W64 path)."""
    X, y, W, o, v = _inputs(link, 60, 6, 3, 1)
    _, G = ref.data_pass(link, X, y, W, o, v)

    def ell_of(W64):
        L = X.astype(np.float64) @ W64.T + o.astype(np.float64)[:, None]
        A, _ = glm.log_partition(link, L)
        return (np.where(v > 0, v, 0.0).astype(np.float64)[:, None] * (y.astype(np.float64)[:, None] * L - A)).sum(axis=0)

    h = 1e-6
    W64 = W.astype(np.float64)
    for s in range(3):
        for d in range(6):
            e = np.zeros_like(W64)
            e[s, d] = h
            fd = (ell_of(W64 + e)[s] - ell_of(W64 - e)[s]) / (2 * h)
            npt.assert_allclose(G[s, d], fd, rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("link", LINKS)
def test_reference_without_offset_and_weights_is_the_shipped_reference(link):
    X, y, W, _, _ = _inputs(link, 300, 8, 4, 2)
    B = X.shape[0]
    want = glm.glm_data_pass(link, X, y, W)
    for o, v in ((None, None), (np.zeros(B, np.float32), None), (None, np.ones(B, np.float32)),
                 (np.zeros(B, np.float32), np.ones(B, np.float32))):
        got = ref.data_pass(link, X, y, W, o, v)
        npt.assert_allclose(got[0], want[0], rtol=1e-14)
        npt.assert_allclose(got[1], want[1], rtol=1e-13, atol=1e-13)


def test_binomial_rows_equal_their_expansion():
    """(x, y = k / n, v = n) gives the same ell and G as the n Bernoulli rows (k ones, n - k zeros)."""
    rs = np.random.RandomState(3)
    B, D, S = 40, 8, 3
    X, _, W, o, _ = _inputs("logistic", B, D, S, 3)
    n = rs.randint(1, 9, B)
    k = rs.binomial(n, 0.4)
    agg = ref.data_pass("logistic", X, (k / n).astype(np.float32).astype(np.float64), W, o, n.astype(np.float32))
    # y = k / n is not a float32 in general: compare in float64 with the exact ratio
    L = ref.logits(X, W, o)
    A, dA = glm.log_partition("logistic", L)
    y64 = (k / n)[:, None]
    ell = (n[:, None] * (y64 * L - A)).sum(axis=0)
    G = (n[:, None] * (y64 - dA)).T @ X.astype(np.float64)
    Xe, ye = ref.expand_binomial(X, k, n)
    oe = np.repeat(o, n)
    exp_ = ref.data_pass("logistic", Xe, ye, W, oe, None)
    npt.assert_allclose(ell, exp_[0], rtol=1e-12)
    npt.assert_allclose(G, exp_[1], rtol=1e-11, atol=1e-12)
    # and the float32-rounded y of the aggregated rows moves it by float32 rounding only
    npt.assert_allclose(agg[0], exp_[0], rtol=1e-6)


def test_zero_weight_rows_are_dropped_by_a_select():
    X, y, W, o, v = _inputs("poisson", 50, 8, 3, 4)
    o[5], v[5] = 200.0, 0.0
    o[6], v[6] = 300.0, 0.0
    ell, G = ref.data_pass("poisson", X, y, W, o, v)
    assert np.isfinite(ell).all() and np.isfinite(G).all()
    keep = v > 0
    want = ref.data_pass("poisson", X[keep], y[keep], W, o[keep], v[keep])
    npt.assert_allclose(ell, want[0], rtol=1e-14)
    npt.assert_allclose(G, want[1], rtol=1e-13, atol=1e-13)
    assert np.isfinite(ref.ell_bound("poisson", X, y, W, o, v)).all()


@pytest.mark.parametrize("B,D,S", [(37, 8, 3), (2051, 256, 8), (4099, 64, 5)])
@pytest.mark.parametrize("link", LINKS)
def test_a_naive_float32_evaluation_lies_inside_the_device_bounds(link, B, D, S):
    """Serial float32 sums, row after row: ell within 2e-5 of sum_n v_n (|y l| + A + 1), G within 1e-4 of max|G|, the
    bounds the device pass is held to (measured here: at most 5.2e-7 and 1.6e-6, a factor of about 40 inside)."""
    X, y, W, o, v = _inputs(link, B, D, S, B + D)
    ell, G = ref.data_pass_f32(link, X, y, W, o, v)
    ell_r, G_r = ref.data_pass(link, X, y, W, o, v)
    bound = ref.ell_bound(link, X, y, W, o, v)
    e_ell = (np.abs(ell - ell_r) / bound).max()
    e_G = np.abs(G - G_r).max() / np.abs(G_r).max()
    print("%s (%d, %d, %d): ell err/bound %.3g, G err/max %.3g" % (link, B, D, S, e_ell, e_G))
    assert e_ell <= 2e-5 and e_G <= 1e-4


# ---- drivers: argument errors before any device call -----------------------------------------------------------------

def _host_batch(B=12, D=8):
    return torch.zeros((B, D), dtype=torch.float32), torch.zeros(B, dtype=torch.float32)


class _NoDevice:
    """A context that fails the test when the driver touches it."""

    def __getattr__(self, name):
        raise AssertionError("the driver reached for the device (ctx.%s) before refusing its arguments" % name)


def test_driver_argument_errors_come_before_any_device_call():
    from bayesic_amd.svi import GLMReparamSVI
    X, y = _host_batch()
    ones = torch.ones(12, dtype=torch.float32)
    ctx = _NoDevice()
    with pytest.raises(ValueError, match="exposure belongs to the Poisson"):
        GLMReparamSVI(X, y, link="logistic", exposure=ones, ctx=ctx)
    with pytest.raises(ValueError, match="mutually exclusive"):
        GLMReparamSVI(X, y, link="poisson", exposure=ones, offset=ones, ctx=ctx)
    with pytest.raises(ValueError, match=r"offset must be \[12\]"):
        GLMReparamSVI(X, y, link="poisson", offset=torch.ones(11), ctx=ctx)
    with pytest.raises(ValueError, match=r"weights must be \[12\]"):
        GLMReparamSVI(X, y, link="logistic", weights=torch.ones((12, 1)), ctx=ctx)
    with pytest.raises(TypeError, match="offset must be float32"):
        GLMReparamSVI(X, y, link="poisson", offset=ones.double(), ctx=ctx)
    with pytest.raises(TypeError, match="weights must be float32"):
        GLMReparamSVI(X, y, link="poisson", weights=ones.double(), ctx=ctx)
    with pytest.raises(ValueError, match="strictly positive"):
        GLMReparamSVI(X, y, link="poisson", exposure=torch.zeros(12), ctx=ctx)
    with pytest.raises(ValueError, match="finite and >= 0"):
        GLMReparamSVI(X, y, link="poisson", weights=-ones, ctx=ctx)
    with pytest.raises(ValueError, match="finite and >= 0"):
        GLMReparamSVI(X, y, link="poisson", weights=ones * float("nan"), ctx=ctx)
    with pytest.raises(ValueError, match="contiguous"):
        GLMReparamSVI(X, y, link="poisson", offset=torch.ones(24)[::2], ctx=ctx)


def test_predict_refuses_an_offset_model_without_an_offset():
    from bayesic_amd.svi.predict import heldout_lpd, predict
    X, y = _host_batch()
    model = types.SimpleNamespace(link="poisson", has_offset=True, ctx=_NoDevice(), D=8)
    with pytest.raises(ValueError, match="fitted with an offset"):
        predict(model, X)
    with pytest.raises(ValueError, match="fitted with an offset"):
        heldout_lpd(model, X, y, weights=torch.ones(12))
    plain = types.SimpleNamespace(link="logistic", has_offset=False, ctx=_NoDevice(), D=8)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson"):
        predict(plain, X, exposure=torch.ones(12))
    gauss = types.SimpleNamespace(family=None, ctx=_NoDevice(), D=8)
    with pytest.raises(ValueError, match="logistic and Poisson models"):
        predict(gauss, X, offset=torch.ones(12))


def test_keywords_and_entry_points_are_declared():
    import inspect
    from bayesic_amd import _ffi
    from bayesic_amd.svi import GLMReparamSVI
    from bayesic_amd.svi.predict import heldout_lpd, predict
    for fn in (GLMReparamSVI.__init__, GLMReparamSVI.predict, GLMReparamSVI.heldout_lpd, predict, heldout_lpd):
        names = inspect.signature(fn).parameters
        assert {"offset", "weights", "exposure"} <= set(names), fn
    assert {"offset", "weights"} <= set(inspect.signature(GLMReparamSVI.set_batch).parameters)
    sig = _ffi.SIGNATURES
    assert len(sig["bsc_glm_data_pass_obs"][1]) == len(sig["bsc_glm_data_pass"][1]) + 2
    assert len(sig["bsc_glm_pass_update_obs"][1]) == len(sig["bsc_glm_pass_update"][1]) + 2
    assert len(sig["bsc_predict_pass_offset"][1]) == len(sig["bsc_predict_pass"][1]) + 1
    header = open(_ffi.os.path.join(_ffi.os.path.dirname(_ffi._HERE), "include", "bayesic_hip.h")).read()
    for name in ("bsc_glm_data_pass_obs", "bsc_glm_pass_update_obs", "bsc_predict_pass_offset"):
        assert "int %s(bsc_ctx* ctx" % name in header
