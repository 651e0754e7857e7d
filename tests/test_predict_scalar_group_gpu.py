"""GPU checks of the predictive of the random-intercept models with a learned scalar
(csrc/bsc_predict_scalar_group.hip through the C ABI, svi/hier_scalar.py, svi/predict.py) against
tests/_glm_scalar_group_ref.py, which feeds the one-hot design (the unseen group as column J) to the family's own
predict and predict_bounds: every output lies inside the family's bounds, nothing wider.  A zero table is compared with
the family's ungrouped predictive with ==.

Shapes: B in {1, 17, 37, 1003}, D in {8, 64, 252, 256}, J in {1, 3, 1000}, S in {8, 24, 40} (one, two and four
accumulator chunks of sixteen draws), ids of -1 among the rows, ids four bytes off alignment, with and without an
offset; logits kept at |l| <= 3.5 (the predictive mean is exp(l)), tau inside each family's envelope.

The end-to-end fits are tests/_glm_scalar_group_ref.py's simulated data set (3000 rows, D = 8, J = 20, intercept
spread 0.8): tests/test_glm_scalar_group_cpu.py shows in float64 that known groups beat id -1 and the grouped model
beats the ungrouped one by more than 0.05 nats per held-out row; here the same inequalities are asserted on the device
with the drivers themselves."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_scalar_group_ref as ref

pytestmark = pytest.mark.gpu

FAMILIES = ref.FAMILIES
CODE = ref.CODE
UNGROUPED = {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass", "weibull": "bsc_weibull_predict_pass"}
SENTINEL = 1.0e30


def _dev_vec(ctx, a, shift=False, guard=16, dtype=np.float32, sentinel=SENTINEL):
    if a is None:
        return None
    buf = np.concatenate([[sentinel] if shift else [], a, np.full(guard, sentinel)]).astype(dtype)
    t = ctx.to_device(buf)
    return t[1:1 + len(a) + guard] if shift else t


def _outputs(ctx, B):
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    return out


def _predict(ctx, fam, X, y, g, J, W, Bt, logtau, o, shift=False):
    B, D = X.shape
    S = W.shape[0]
    out = _outputs(ctx, B)
    gd = _dev_vec(ctx, g, shift, dtype=np.int32, sentinel=-2)
    ctx.call("bsc_scalar_predict_pass_groups", CODE[fam], ctx.to_device(X), D, _dev_vec(ctx, y), _dev_vec(ctx, o, shift),
             gd, B, D, J, ctx.to_device(W), ctx.to_device(Bt), Bt.shape[1], _dev_vec(ctx, logtau, shift), S,
             out["mean"], out["var"], out["lpd"], out["lpd_sum"])
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _inputs(fam, B, D, J, S, seed, offset=True):
    """X ~ N / sqrt(D), W ~ 0.6 N, Bm and b_new ~ 0.5 N, offsets N(0, 1), all scaled so that |l| <= 3.5; one id in
    four is -1; y from the family at the first draw's logit (weibull: three in ten censored)."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    Bm = (0.5 * rs.standard_normal((S, J))).astype(np.float32)
    b_new = (0.5 * rs.standard_normal(S)).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    g[rs.uniform(size=B) < 0.25] = -1
    o = rs.standard_normal(B).astype(np.float32) if offset else None
    g1, B1 = ref._with_new(g, J, Bm, b_new)
    peak = np.abs(ref.grp.logits(X, g1, W, B1, o)).max()
    if peak > 3.5:
        W, Bm, b_new = ((a * (3.5 / peak)).astype(np.float32) for a in (W, Bm, b_new))
        o = None if o is None else (o * (3.5 / peak)).astype(np.float32)
        g1, B1 = ref._with_new(g, J, Bm, b_new)
    lo, hi = ref.TAU_RANGE[fam]
    logtau = (np.linspace(lo, hi, S)[rs.permutation(S)] if S > 1 else np.array([0.5])).astype(np.float32)
    l0 = ref.grp.logits(X, g1, W, B1, o)[:, 0]
    if fam == "negbin":
        y = rs.negative_binomial(2, 2.0 / (2.0 + np.exp(l0))).astype(np.float64)
    elif fam == "gamma":
        y = np.maximum(rs.gamma(2.0, np.exp(l0) / 2.0), 1e-30)
    else:
        t = np.maximum(np.exp(l0) * rs.weibull(1.5, B), 1e-30)
        y = np.where(rs.uniform(size=B) < 0.3, -t * rs.uniform(0.1, 1.0, B), t)
        k = np.exp(logtau.astype(np.float64))[None, :]
        # z <= 60 on every (row, draw), as in the pass's tests
        over = (np.log(np.abs(y))[:, None] - ref.grp.logits(X, g1, W, B1, o) - 60.0 / k).max()
        y = y * math.exp(-max(over, 0.0) - 1e-3)
    return X, y.astype(np.float32), g, W, Bm, b_new, logtau, o


def _assert_predict(fam, got, X, y, g, J, W, Bm, b_new, logtau, o):
    want = ref.predict(fam, X, g, J, W, Bm, b_new, logtau, y, o)
    bnd = ref.predict_bounds(fam, X, g, J, W, Bm, b_new, logtau, y, o)
    for k in ("mean", "var", "lpd", "lpd_sum"):
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        print("%s B=%d D=%d J=%d S=%d %s: worst error / bound %.3g" % (fam, X.shape[0], X.shape[1], J, W.shape[0], k,
                                                                        worst))
        assert worst <= 1.0, (k, worst)


@pytest.mark.parametrize("S", [8, 24, 40])
@pytest.mark.parametrize("D", [8, 64, 252, 256])
@pytest.mark.parametrize("fam", FAMILIES)
def test_predictive_lies_inside_the_familys_bounds(ctx, fam, D, S):
    for B, J, offset in ((1, 1, True), (17, 3, False), (37, 1000, True), (1003, 3, True), (1003, 1000, False)):
        X, y, g, W, Bm, b_new, logtau, o = _inputs(fam, B, D, J, S, seed=B + D + S + J, offset=offset)
        got = _predict(ctx, fam, X, y, g, J, W, ref.table(Bm, b_new), logtau, o, shift=(B == 37))
        _assert_predict(fam, got, X, y, g, J, W, Bm, b_new, logtau, o)


@pytest.mark.parametrize("D,S", [(256, 40), (64, 8), (252, 24)])
@pytest.mark.parametrize("fam", FAMILIES)
def test_a_zero_table_is_the_ungrouped_predictive_bit_for_bit(ctx, fam, D, S):
    B, J = 1003, 9
    X, y, g, W, Bm, b_new, logtau, o = _inputs(fam, B, D, J, S, seed=D + S)
    got = _predict(ctx, fam, X, y, g, J, W, ref.table(0 * Bm, 0 * b_new), logtau, o)
    out = _outputs(ctx, B)
    ctx.call(UNGROUPED[fam], ctx.to_device(X), D, _dev_vec(ctx, y), _dev_vec(ctx, o), B, D, ctx.to_device(W),
             _dev_vec(ctx, logtau), S, out["mean"], out["var"], out["lpd"], out["lpd_sum"])
    ctx.sync()
    for k, t in out.items():
        npt.assert_array_equal(got[k], t.cpu().numpy(), err_msg=k)


def test_refusals_name_the_entry_point_and_leave_the_outputs_alone(ctx):
    from bayesic_amd._ffi import BayesicHipError
    who = "bsc_scalar_predict_pass_groups"
    X, y, W, lt = ctx.zeros((8, 64)), ctx.zeros(8), ctx.zeros((8, 64)), ctx.zeros(8)
    g = torch.zeros(8, dtype=torch.int32, device=ctx.device)
    Bt = ctx.zeros((4, 16))
    out = _outputs(ctx, 8)

    def call(fam=0, J=3, ldb=16, lta=lt, Bta=Bt, ga=g):
        ctx.call(who, fam, X, 64, y, None, ga, 8, 64, J, W, Bta, ldb, lta, 8, out["mean"], out["var"], out["lpd"],
                 out["lpd_sum"])

    with pytest.raises(BayesicHipError, match=who + ": family=5 must be BSC_SCALAR_NEGBIN"):
        call(fam=5)
    with pytest.raises(BayesicHipError, match=who + ": logtau is null"):
        call(lta=None)
    with pytest.raises(BayesicHipError, match=who + ": groups and Bt must not be null"):
        call(ga=None)
    with pytest.raises(BayesicHipError, match=who + ": J=0 must be in"):
        call(J=0)
    with pytest.raises(BayesicHipError, match=who + ": ldb=6 must be >= S"):
        call(ldb=6)
    with pytest.raises(BayesicHipError, match=who + ": Bt must be 16-byte aligned"):
        call(Bta=Bt.view(-1)[1:])
    ctx.sync()
    for t in out.values():
        assert (t.cpu().numpy() == -777.0).all()
    bad = torch.tensor([0, 1, -1, 3, 1, 0, 0, 0], dtype=torch.int32, device=ctx.device)
    with pytest.raises(BayesicHipError, match=r"row 3 has group id 3 outside \[-1,3\)"):
        ctx.call("bsc_group_ids_check", bad, 8, 3, 1)


# ---- the drivers' predict() against the reference, and the end-to-end fits ------------------------------------------------

def _driver(fam, ctx, data, **kw):
    from bayesic_amd.svi import HierGammaReparamSVI, HierNegBinReparamSVI, HierWeibullReparamSVI
    X, y, g = data["X"], data["y"], data["g"]
    if fam == "weibull":
        return HierWeibullReparamSVI(X, np.abs(y), g, ref.FIT["J"], event=y > 0, ctx=ctx, **kw)
    cls = HierNegBinReparamSVI if fam == "negbin" else HierGammaReparamSVI
    return cls(X, y, g, ref.FIT["J"], ctx=ctx, **kw)


def _ungrouped_driver(fam, ctx, data, **kw):
    from bayesic_amd.svi import GammaReparamSVI, NegBinReparamSVI, WeibullReparamSVI
    X, y = data["X"], data["y"]
    if fam == "weibull":
        return WeibullReparamSVI(X, np.abs(y), y > 0, ctx=ctx, **kw)
    return (NegBinReparamSVI if fam == "negbin" else GammaReparamSVI)(X, y, ctx=ctx, **kw)


def _lpd(fam, model, data, groups=None):
    X, y = data["X_test"], data["y_test"]
    kw = dict(n_samples=ref.FIT["S_pred"]) if groups is None else dict(groups=groups, n_samples=ref.FIT["S_pred"])
    if fam == "weibull":
        return model.heldout_lpd(X, np.abs(y), y > 0, **kw)
    return model.heldout_lpd(X, y, **kw)


@pytest.mark.parametrize("fam", FAMILIES)
def test_fit_known_groups_beat_new_ones_and_the_grouped_model_beats_the_ungrouped(ctx, fam):
    from bayesic_amd.svi import posterior_draws
    F = ref.FIT
    data = ref.simulate(fam)
    kw = dict(n_samples=F["S"], seed=F["seed"], lr=F["lr"])
    model, flat = _driver(fam, ctx, data, **kw), _ungrouped_driver(fam, ctx, data, **kw)
    for _ in range(F["steps"]):
        model.step()
        flat.step()
    ctx.sync()
    g_test = data["g_test"]
    known = _lpd(fam, model, data, g_test)
    new = _lpd(fam, model, data, np.full(len(g_test), -1, np.int32))
    ungrouped = _lpd(fam, flat, data)
    p = model.params()
    spread = math.exp(-0.5 * p["zeta"][0])
    print("%s: held-out lpd known %.4f, new groups %.4f, ungrouped %.4f; spread %.3f, %s" % (
        fam, known, new, ungrouped, spread, {k: v for k, v in p.items() if k.endswith("_mean")}))
    assert known > new and known > ungrouped
    assert abs(spread - F["spread"]) < F["spread"] / 3.0
    # the driver's draws and predict() are the reference's at the driver's own lam
    lam = model.lam.cpu().numpy()
    W, Bm, b_new, logtau = ref.posterior_draws(lam, F["D"], F["J"], F["S_pred"], F["seed"])
    Wd, Btd, ltd = posterior_draws(model, F["S_pred"])
    npt.assert_array_equal(Wd.cpu().numpy(), W)
    npt.assert_array_equal(Btd.cpu().numpy(), ref.table(Bm, b_new))
    npt.assert_array_equal(ltd.cpu().numpy(), logtau)
    ids = g_test.copy()
    ids[::3] = -1
    X, y = data["X_test"], data["y_test"]
    if fam == "weibull":
        out = model.predict(X, np.abs(y), y > 0, groups=ids, n_samples=F["S_pred"])
        surv = model.survival(X, np.abs(y), groups=ids, n_samples=F["S_pred"]).cpu().numpy()
        want_s = np.exp(ref.predict(fam, X, ids, F["J"], W, Bm, b_new, logtau, -np.abs(y))["lpd"])
        b_s = ref.predict_bounds(fam, X, ids, F["J"], W, Bm, b_new, logtau, -np.abs(y))["lpd"]
        assert (np.abs(surv - want_s) <= want_s * np.expm1(b_s) + 1e-6).all()      # exp of an lpd inside its bound
    else:
        out = model.predict(X, y, groups=ids, n_samples=F["S_pred"])
    _assert_predict(fam, {k: t.cpu().numpy() for k, t in out.items()}, X, y, ids, F["J"], W, Bm, b_new, logtau, None)
