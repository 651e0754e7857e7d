"""No device: the float64 restatement of the grouped predictive (tests/_predict_group_ref.py) against scipy.stats and
against tests/_predict_ref.py on the one-hot design, the layout of the intercept table, the draw of a group that was
not seen in training, a float32 evaluation inside the bounds the GPU tests use (at their shapes), and the Python
layer's refusals that need no device."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy import stats

import _glm_group_ref as grp
import _predict_group_ref as ref
import _predict_ref as pref


def _inputs(family, B, D, J, S, seed, with_offset=True):
    """tests/test_predict_group_gpu._inputs, restated (that module imports torch and is marked gpu)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    b = (0.5 * rs.standard_normal((S, J))).astype(np.float32)
    b_new = (0.8 * rs.standard_normal(S)).astype(np.float32)
    g = rs.randint(-1, J, size=B).astype(np.int32)
    o = rs.standard_normal(B).astype(np.float32) if with_offset else None
    if family == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, g, W, ref.table(b, b_new), o)).max()
        if peak > 3.5:
            W, b, b_new = ((a * (3.5 / peak)).astype(np.float32) for a in (W, b, b_new))
            o = None if o is None else (o * (3.5 / peak)).astype(np.float32)
    return X, y, g, W, ref.table(b, b_new), o


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_the_reference_is_scipy_log_pmf_and_the_one_hot_design(family):
    B, D, J, S = 203, 8, 5, 17
    X, y, g, W, Bt, o = _inputs(family, B, D, J, S, seed=1)
    assert (g == -1).any() and (g == J - 1).any()
    L = ref.logits(X, g, W, Bt, o)
    # the logits, term by term
    rows = np.where(g == -1, J, g)
    for n in (0, 7, B - 1):
        for s in (0, S - 1):
            want = float(X[n].astype(np.float64) @ W[s].astype(np.float64)) + float(Bt[rows[n], s]) + float(o[n])
            assert abs(L[n, s] - want) < 1e-12
    # log p(y | l) of every draw against scipy.stats, then the log-mean-exp
    if family == "logistic":
        lp = stats.bernoulli.logpmf(y[:, None], 1.0 / (1.0 + np.exp(-L)))
        mu, v = 1.0 / (1.0 + np.exp(-L)), np.exp(-L) / (1.0 + np.exp(-L)) ** 2
    else:
        lp = stats.poisson.logpmf(y[:, None], np.exp(L))
        mu, v = np.exp(L), np.exp(L)
    out = ref.predict(family, X, g, W, Bt, y, o)
    npt.assert_allclose(out["lpd"], np.log(np.exp(lp).mean(axis=1)), rtol=1e-10)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-14)
    npt.assert_allclose(out["mean"], mu.mean(axis=1), rtol=1e-12)
    npt.assert_allclose(out["var"], v.mean(axis=1) + mu.var(axis=1), rtol=1e-10)
    # the one-hot design [X | onehot(row(g))] against [W | b | b_new], offset left out: tests/_predict_ref.py's model
    X1 = np.concatenate([X, grp.onehot(rows, J + 1)], axis=1)
    W1 = np.concatenate([W, Bt[:, :S].T], axis=1)
    a, b = ref.predict(family, X, g, W, Bt, y), pref.predict(family, X1, W1, None, y)
    for k in a:
        npt.assert_allclose(a[k], b[k], rtol=1e-11, atol=1e-13)
    # ... and their bounds agree where the models do (the one-hot column's |x w| is the intercept's magnitude)
    ba, bb = ref.bounds(family, X, g, W, Bt, y), pref.bounds(family, X1, W1, None, y)
    for k in ba:
        npt.assert_allclose(ba[k], bb[k], rtol=1e-9)


def test_the_stable_logistic_variance_at_large_logits():
    L = np.array([[-80.0, -37.0, 0.0, 37.0, 80.0]])
    mu, v = ref.moments("logistic", L)
    npt.assert_allclose(v[0], np.exp(-np.abs(L[0])) / (1.0 + np.exp(-np.abs(L[0]))) ** 2, rtol=1e-14)
    assert (v > 0).all() and pref.moments("logistic", L)[1][0, -1] == 0.0       # what the shared form loses


@pytest.mark.parametrize("S,ld", [(1, 16), (8, 16), (16, 16), (17, 32), (33, 48), (64, 64)])
def test_the_layout_of_the_intercept_table(S, ld):
    from bayesic_amd.svi import predict as mod
    J = 5
    rs = np.random.RandomState(S)
    b, b_new = rs.standard_normal((S, J)), rs.standard_normal(S)
    assert mod.table_ld(S) == ref.table_ld(S) == ld
    for Bt in (ref.table(b, b_new), mod.intercept_table(b.astype(np.float32), b_new.astype(np.float32))):
        assert Bt.shape == (J + 1, ld) and Bt.dtype == np.float32 and Bt.flags["C_CONTIGUOUS"]
        npt.assert_array_equal(Bt[:J, :S], b.T.astype(np.float32))
        npt.assert_array_equal(Bt[J, :S], b_new.astype(np.float32))
        assert (Bt[:, S:] == 0).all()
    npt.assert_array_equal(ref.rows_of(np.array([-1, 0, J - 1]), J), [J, 0, J - 1])


def test_the_new_group_draw_is_a_normal_of_the_drawn_precision():
    """b_new,s = e^{-zeta_s / 2} eps_s with zeta_s ~ q(zeta): against a direct Monte-Carlo of N(0, e^{-zeta})."""
    D, J, S = 4, 3, 64
    P = D + J + 1
    lam = np.zeros(2 * P)
    lam[P - 1], lam[2 * P - 1] = 1.2, math.log(0.3)            # q(zeta) = N(1.2, 0.3^2)
    lam[P:2 * P - 1] = math.log(0.1)
    draws = np.concatenate([ref.posterior_draws(lam, D, J, S, seed)[1][J, :S] for seed in range(400)])
    # the formula, on the same noise
    from oracle import philox
    eps = philox.normal_draws(7, S, P + 1, stream=pref.STREAM, step=0)
    zeta = lam[P - 1] + math.exp(lam[2 * P - 1]) * eps[:, P - 1]
    npt.assert_allclose(ref.posterior_draws(lam, D, J, S, 7)[1][J, :S], np.exp(-0.5 * zeta) * eps[:, P], rtol=1e-6)
    # its law: mean 0, variance E e^{-zeta} = exp(-m + s^2 / 2), checked against numpy's own draws of the same mixture
    rs = np.random.RandomState(0)
    direct = rs.standard_normal(draws.size) * np.exp(-0.5 * (1.2 + 0.3 * rs.standard_normal(draws.size)))
    var = math.exp(-1.2 + 0.5 * 0.09)
    n = draws.size
    assert abs(draws.mean()) < 4.0 * math.sqrt(var / n) and abs(direct.mean()) < 4.0 * math.sqrt(var / n)
    kurt = 3.0 * math.exp(0.09)                                  # E b^4 / var^2 of the scale mixture
    se = var * math.sqrt((kurt - 1.0) / n)
    assert abs(draws.var() - var) < 4.0 * se and abs(direct.var() - var) < 4.0 * se
    assert stats.ks_2samp(draws, direct).pvalue > 1e-3


@pytest.mark.parametrize("D", [4, 132, 256])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_a_float32_evaluation_is_inside_the_bounds_at_the_gpu_shapes(family, D):
    worst = 0.0
    for S in (1, 17, 64):
        for B, J, with_offset in ((1, 1, False), (17, 5, True), (325, 1000, True)):
            X, y, g, W, Bt, o = _inputs(family, B, D, J, S, seed=B * 7 + D + S + J, with_offset=with_offset)
            want, got = ref.predict(family, X, g, W, Bt, y, o), ref.predict_f32(family, X, g, W, Bt, y, o)
            bnd = ref.bounds(family, X, g, W, Bt, y, o)
            for k in want:
                r = float(np.max(np.abs(got[k] - want[k]) / bnd[k]))
                assert r <= 1.0, (S, B, J, k, r)
                worst = max(worst, r)
    assert worst > 1e-4          # the float32 evaluation is a float32 evaluation


def test_the_extremes_of_the_gpu_tests_are_inside_their_bounds_in_float32():
    J, S = 3, 8
    g = (np.arange(40) % (J + 1) - 1).astype(np.int32)
    y = ((np.arange(40) // (J + 1)) % 2).astype(np.float32)
    X, W = np.zeros((40, 8), np.float32), np.zeros((S, 8), np.float32)
    for family, top in (("logistic", 80.0), ("poisson", 4.0)):
        Bt = np.zeros((J + 1, 16), np.float32)
        Bt[0, :S], Bt[1, :S], Bt[J, :S] = top, -top, -top
        want, got = ref.predict(family, X, g, W, Bt, y), ref.predict_f32(family, X, g, W, Bt, y)
        bnd = ref.bounds(family, X, g, W, Bt, y)
        for k in want:
            assert np.isfinite(got[k]).all() and (np.abs(got[k] - want[k]) <= bnd[k]).all(), (family, k)


# ---- the Python layer, without a device -----------------------------------------------------------------------------

def test_missing_groups_are_refused_not_read_as_new_groups():
    from bayesic_amd.svi.hier_glm import HierGLMReparamSVI, check_predict_groups
    with pytest.raises(NotImplementedError, match="per-draw, per-group term.*pass groups="):
        check_predict_groups(None, 5)
    X = np.zeros((5, 4), np.float32)
    for method in (HierGLMReparamSVI.predict, HierGLMReparamSVI.heldout_lpd):     # before anything of the driver is read
        with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
            method(None, X, np.zeros(5, np.float32))


def test_wrong_dtype_or_length_of_groups_is_refused():
    import torch
    from bayesic_amd.svi.hier_glm import check_predict_groups
    check_predict_groups(np.zeros(5, np.int32), 5)
    check_predict_groups(np.array([0, -1, 2, 3, 4]), 5)          # host integers are uploaded as int32
    check_predict_groups(torch.zeros(5, dtype=torch.int32), 5)
    check_predict_groups(12345678, 5)                            # a raw device pointer is taken as it is
    with pytest.raises(TypeError, match="int32"):
        check_predict_groups(torch.zeros(5, dtype=torch.int64), 5)
    with pytest.raises(TypeError, match="integers"):
        check_predict_groups(np.zeros(5, np.float32), 5)
    with pytest.raises(ValueError, match=r"contiguous \[5\]"):
        check_predict_groups(np.zeros(4, np.int32), 5)
    with pytest.raises(ValueError, match=r"contiguous \[5\]"):
        check_predict_groups(torch.zeros((5, 1), dtype=torch.int32), 5)
    with pytest.raises(ValueError, match=r"contiguous \[5\]"):
        check_predict_groups(torch.zeros(10, dtype=torch.int32)[::2], 5)


def test_groups_on_another_model_or_route_is_a_value_error():
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.svi import predict as mod

    class Plain:                       # what svi/predict.py reads of a driver without groups
        link, D = "logistic", 4
    with pytest.raises(ValueError, match="random-intercept model"):
        mod.predict(Plain(), np.zeros((3, 4), np.float32), groups=np.zeros(3, np.int32))
    # a route without a driver: the general one on the host backend (tests/test_predict_cpu.py's engine)
    from oracle.einsum_eval import NumpyBackend
    from bayesic_amd.inference.models import logistic_regression_log_joint
    rs = np.random.RandomState(0)
    X = rs.standard_normal((50, 4))
    y = (rs.uniform(size=50) < 0.5) * 1.0
    lj, v = logistic_regression_log_joint(1.0, 1.0)
    eng = ReparamVI(lj, [(v["W"], 4)], dict(X=X, y=y), n_samples=4, seed=1, backend=NumpyBackend(np.float64))
    assert eng.route == "general"
    with pytest.raises(ValueError, match="random-intercept route"):
        eng.predict(X, groups=np.zeros(50, np.int32))
    with pytest.raises(NotImplementedError, match="route 'general'"):
        eng.predict(X)


def test_the_signatures_carry_groups():
    import inspect
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi.hier_glm import HierGLMReparamSVI
    assert list(inspect.signature(HierGLMReparamSVI.predict).parameters) == [
        "self", "X", "y", "groups", "n_samples", "seed", "draws", "offset", "exposure", "weights"]
    for fn in (mod.predict, mod.heldout_lpd, ReparamVI.predict, HierGLMReparamSVI.heldout_lpd):
        assert inspect.signature(fn).parameters["groups"].default is None
