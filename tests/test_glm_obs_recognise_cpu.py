"""``recognise.glm_linear`` with an offset and row weights: the builders' models and other writings of them are read
with the right roles, scale and tau; a coefficient on the offset that is not 1 and a weight inside the link are declined
with a reason.  (The recognitions and declines without these vectors are tests/test_glm_cpu.py's, unchanged.)"""
import numpy as np
import numpy.testing as npt
import pytest

from bayesic_amd import algebra as A
from bayesic_amd.inference import recognise as R
from bayesic_amd.inference.models import logistic_regression_log_joint, poisson_regression_log_joint

N, D, S = 1000, 16, 8
BUILDERS = {"logistic": logistic_regression_log_joint, "poisson": poisson_regression_log_joint}


def _shapes(names):
    return dict({"X": (N, D)}, **{n: (N,) for n in names})


@pytest.mark.parametrize("offset,weights", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("link", sorted(BUILDERS))
def test_the_builders_are_recognised_with_their_roles(link, offset, weights):
    scale, tau = 37.5, 2.5
    lj, v = BUILDERS[link](scale, tau, offset=offset, weights=weights)
    assert ("offset" in v) == offset and ("weights" in v) == weights
    names = ["y"] + (["offset"] if offset else []) + (["weights"] if weights else [])
    why = []
    plan = R.glm_linear(lj, [(v["W"], D)], _shapes(names), S, why=why)
    assert plan is not None, why
    assert (plan.link, plan.X, plan.y, plan.W) == (link, "X", "y", "W")
    assert plan.offset == ("offset" if offset else None) and plan.weights == ("weights" if weights else None)
    npt.assert_allclose([plan.scale, plan.tau], [scale, tau], rtol=1e-9)


@pytest.mark.parametrize("link", sorted(BUILDERS))
def test_the_defaults_build_the_model_without_them(link):
    lj, v = BUILDERS[link](3.0, 1.5)
    assert sorted(v) == ["W", "X", "y"] and sorted(lj.input_types) == ["W", "X", "y"]
    plan = R.glm_linear(lj, [(v["W"], D)], _shapes(["y"]), S)
    assert plan is not None and plan.offset is None and plan.weights is None


def _written(link, X, W, y, o, v, scale, tau, o_coef=1.0, weight_inside=False):
    """Other names, another order: the weights multiply each of the two terms, the offset is added on the left."""
    l = A.dimshuffle(o, "x", 0) * o_coef + A.dot(W, X.T) if o_coef != 1.0 else A.dimshuffle(o, "x", 0) + A.dot(W, X.T)
    vb, yb = A.dimshuffle(v, "x", 0), A.dimshuffle(y, "x", 0)
    inner = l * vb if weight_inside else l
    part = A.log(1.0 + A.exp(inner)) if link == "logistic" else A.exp(inner)
    data = A.sum(vb * yb * l * scale, axis=1) - A.sum(part * vb, axis=1) * scale
    return data + A.sum(W * W, axis=1) * (-0.5 * tau) + 1.5


def _vars():
    # the alphabetical order of the names is not the order of the roles
    return A.var("design", 2), A.var("beta", 2), A.var("zz_counts", 1), A.var("log_exposure", 1), A.var("a_freq", 1)


@pytest.mark.parametrize("link", sorted(BUILDERS))
def test_other_names_and_another_order_are_recognised(link):
    X, W, y, o, v = _vars()
    scale, tau = 12.0, 0.75
    lj = _written(link, X, W, y, o, v, scale, tau)
    shapes = {"design": (N, D), "zz_counts": (N,), "log_exposure": (N,), "a_freq": (N,)}
    why = []
    plan = R.glm_linear(lj, [(W, D)], shapes, S, why=why)
    assert plan is not None, why
    assert (plan.link, plan.X, plan.y, plan.W, plan.offset, plan.weights) == \
        (link, "design", "zz_counts", "beta", "log_exposure", "a_freq")
    npt.assert_allclose([plan.scale, plan.tau], [scale, tau], rtol=1e-9)


def _declined(lj, W, shapes):
    why = []
    assert R.glm_linear(lj, [(W, D)], shapes, S, why=why) is None
    assert why and why[-1]
    return why[-1]


@pytest.mark.parametrize("link", sorted(BUILDERS))
def test_an_offset_with_a_coefficient_and_a_weight_inside_the_link_are_declined(link):
    X, W, y, o, v = _vars()
    shapes = {"design": (N, D), "zz_counts": (N,), "log_exposure": (N,), "a_freq": (N,)}
    said = _declined(_written(link, X, W, y, o, v, 5.0, 1.0, o_coef=1.7), W, shapes)
    assert "no assignment of the vectors" in said and "coefficient 1" in said
    said = _declined(_written(link, X, W, y, o, v, 5.0, 1.0, weight_inside=True), W, shapes)
    assert "no assignment of the vectors" in said and "outside the link" in said
    # the same with the offset alone
    yb = A.dimshuffle(y, "x", 0)
    l = A.dot(W, X.T) + A.dimshuffle(o, "x", 0) * 1.7
    part = A.log(1.0 + A.exp(l)) if link == "logistic" else A.exp(l)
    lj = A.sum(yb * l - part, axis=1) + A.sum(W * W, axis=1) * (-0.5)
    two = {"design": (N, D), "zz_counts": (N,), "log_exposure": (N,)}
    assert "no assignment of the vectors" in _declined(lj, W, two)
    # a negative scale is still named as such
    l = A.dot(W, X.T) + A.dimshuffle(o, "x", 0)
    part = A.log(1.0 + A.exp(l)) if link == "logistic" else A.exp(l)
    assert "positive" in _declined(A.sum(yb * l - part, axis=1) * (-2.0) + A.sum(W * W, axis=1) * (-0.5), W, two)
    # four vectors are one too many
    u = A.var("extra", 1)
    lj4 = _written(link, X, W, y, o, v, 5.0, 1.0) + A.sum(A.dimshuffle(u, "x", 0) * A.dot(W, X.T), axis=1)
    assert "data inputs" in _declined(lj4, W, dict(shapes, extra=(N,)))
