"""GPU parity of the Weibull route with interval and left censoring (csrc/bsc_glm_weibull_interval.hip through the C ABI,
svi/glm_weibull.py's ``upper=``, svi/predict.py) against the float64 restatement in tests/_glm_weibull_interval_ref.py.

 * ell, T and every entry of G: |dev - ref| <= EPS * bound quantity, EPS = 2e-5 (tests/_glm_weibull_ref.py's value; the
   bound quantities are that reference's docstring).  A plain float32 evaluation stays below 1e-6 of them at these
   shapes, and EPS times them below 1e-3 of the results (tests/test_glm_weibull_interval_cpu.py asserts both);
 * the predictive: tests/_glm_weibull_interval_ref.predict_bounds;
 * five updates against the reference driver: tests/test_glm_weibull_gpu.py's three tolerances (gradient 1e-4 of its
   largest entry, lam atol 2e-4 -- set there for twenty steps, so not loosened by the shorter run --, the ELBO within
   1e-6 of the sum of the sizes of its terms);
 * upper == NULL and two runs: equal bits.

Shapes are the smallest that reach each route: (1003, 12) and (517, 200) the 8-row kernel, narrow and ragged; (1003, 256)
with ``upper`` one float off 16-byte alignment the 8-row D == 256 kernel; (1029, 256) aligned the 16-row MFMA kernel with a
ragged last tile; two batches sized from the device's CU count so that every wave runs two tiles.  S in {3, 8, 11} (11 =
two launches, the second with dead draw slots).  The mixed batch holds about 40 % events, 20 % right-censored, 25 %
interval-censored (widths k d from 1e-4 to 20, every ninth upper end at 1e30) and 15 % left-censored rows; the rows of
weight 0 hold 0, NaN and infinity in y and upper; sentinels of 1e30 behind y, upper, o, v and logshape."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_weibull_interval_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30
PASS, PLAIN = "bsc_glm_weibull_data_pass_interval", "bsc_glm_weibull_data_pass"
WORST = {}


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, upper, W, logshape, o=None, v=None, ld=None, shift=(), name=PASS):
    B, D = X.shape
    S = W.shape[0]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    Wd = ctx.to_device(W)
    yd, ud, od, vd = (_dev_vec(ctx, a, k in shift) for k, a in (("y", y), ("u", upper), ("o", o), ("v", v)))
    pd = _dev_vec(ctx, logshape, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    if name == PASS:
        ctx.call(name, Xd, (ld or D), yd, ud, od, vd, B, D, Wd, pd, S, ell, G, T)
    else:
        ctx.call(name, Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _check(ctx, X, y, upper, W, logshape, o, v, what="", **kw):
    assert ref.TAU_LO <= logshape.min() and logshape.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, upper, W, logshape, o, v, **kw)
    want = ref.data_pass(X, y, upper, W, logshape, o, v)
    bnd = ref.bounds(X, y, upper, W, logshape, o, v)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d: error / tolerance ell %.3g, G %.3g, T %.3g" % (what, X.shape[0], X.shape[1], W.shape[0],
                                                                            *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)
    return got


def _kinds(y, upper, v):
    kept = np.ones(len(y), bool) if v is None else v > 0
    return [int(m[kept].sum()) for m in ((upper == 0) & (y > 0), (upper == 0) & (y < 0), upper > 0, upper < 0)]


# ---- 1. parity at every route, every row kind, null offset and null weight -----------------------------------------------

# leading dimension and shifted vectors of a batch of ref.PASS_BATCHES (default: ld = D, nothing shifted)
LAYOUT = {(1003, 12, 8, "both", "mixed"): (16, ()), (517, 200, 11, "both", "mixed"): (208, ()),
          (1029, 256, 11, "both", "mixed"): (260, ())}


@pytest.mark.parametrize("B,D,S,mode,kinds,ld,shift",
                         [b + LAYOUT.get(b, (None, ())) for b in ref.PASS_BATCHES]
                         + [(1029, 256, 8, "both", "mixed", None, ("u",))])
def test_pass_matches_the_reference(ctx, B, D, S, mode, kinds, ld, shift):
    X, y, upper, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode, kinds=kinds)
    n = _kinds(y, upper, v)
    if kinds == "mixed":
        assert min(n) > 0.1 * sum(n) and (upper == np.float32(ref.FAR)).any()
    else:
        assert n[ref.KINDS.index(kinds) - 1] == sum(n)
    if v is not None:
        dead = v == 0
        assert np.isnan(upper[dead]).any() and np.isinf(upper[dead]).any() and (y[dead] == 0).any()
    got = _check(ctx, X, y, upper, W, logshape, o, v, what="%s %s" % (kinds, mode), ld=ld, shift=shift)
    if kinds in ("event", "right"):     # an all-zero upper: the model of the pass without it, within the two tolerances
        assert (upper[v > 0] == 0).all()
        plain = _pass(ctx, X, np.where(v > 0, y, 1.0).astype(np.float32), None, W, logshape, o, v, name=PLAIN)
        for p, q, bb in zip(got, plain, ref.bounds(X, y, upper, W, logshape, o, v)):
            assert (np.abs(p - q) <= 2.0 * ref.EPS * bb).all()


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D", [(16, 256), (8, 12)])
def test_two_tiles_per_wave_keep_the_upper_ends_with_their_rows(ctx, cu, rows, D):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows, as tests/test_glm_weibull_gpu.py
    builds them: the upper end of the prefetched tile must not reach the tile in flight."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, upper, W, logshape, o, v = ref.make_inputs(B, D, 8, seed=B * 7 + D + 8)
    _check(ctx, X, y, upper, W, logshape, o, v, what="two tiles per wave")


# ---- 2. the same bits: run to run, and with no upper at all -------------------------------------------------------------------

def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (517, 200, 8, 6)):
        X, y, upper, W, logshape, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, upper, W, logshape, o, v)
        b = _pass(ctx, X, y, upper, W, logshape, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


@pytest.mark.parametrize("B,D,S", [(1029, 256, 11), (517, 200, 8)])
def test_a_null_upper_gives_the_bits_of_the_pass_without_it(ctx, B, D, S):
    X, y, W, logshape, o, v = ref.plain_inputs(B, D, S, seed=B + D)    # events and right-censored rows
    a = _pass(ctx, X, y, None, W, logshape, o, v)
    b = _pass(ctx, X, y, None, W, logshape, o, v, name=PLAIN)
    for p, q in zip(a, b):
        npt.assert_array_equal(p, q)
    assert np.abs(b[0]).min() > 0


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_are_the_passes_without_upper_and_upper_is_checked(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9) + 1.0, ctx.zeros((65, 260))
    u, o, v, lp = ctx.zeros(12), ctx.zeros(12), ctx.zeros(12), ctx.zeros(68)
    ell, G, T = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros(65, f64)
    out = ctx.zeros(9)

    def train(ldx, D, S, pa=lp, ua=u):
        ctx.call(PASS, X, ldx, y, ua, o, v, 8, D, W, pa, S, ell, G, T)

    def predict(ldx, D, S, pa=lp, ua=u):
        ctx.call("bsc_weibull_predict_pass_interval", X, ldx, y, ua, o, 8, D, W, pa, S, out, None, None, None)

    for fn, who, code in ((train, PASS, -1), (predict, "bsc_weibull_predict_pass_interval", -3)):
        for args, match in (((12, 10, 8), "%s: D=10 must be a multiple of 4" % who),
                            ((260, 260, 8), "%s: D=260 must be a multiple of 4 in" % who),
                            ((256, 256, 65), "%s: S=65" % who)):
            with pytest.raises(BayesicHipError, match=match) as err:
                fn(*args)
            assert "status %d:" % code in str(err.value), str(err.value)
        with pytest.raises(BayesicHipError, match="%s: logshape is null" % who) as err:
            fn(256, 256, 8, pa=None)
        assert "status -1:" in str(err.value)
        with pytest.raises(BayesicHipError, match="%s: upper must be 4-byte aligned" % who) as err:
            fn(256, 256, 8, ua=u.data_ptr() + 2)
        assert "status -1:" in str(err.value)
    # upper == NULL: the entry points without it refuse, under their own names
    with pytest.raises(BayesicHipError, match="%s: D=10 must be a multiple of 4" % PLAIN):
        train(12, 10, 8, ua=None)
    with pytest.raises(BayesicHipError, match="bsc_weibull_predict_pass: D=10 must be a multiple of 4"):
        predict(12, 10, 8, ua=None)
    ctx.sync()


# ---- 4. the predictive -------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, upper, W, logshape, o, name="bsc_weibull_predict_pass_interval"):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, ud, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, upper, True), _dev_vec(ctx, o), _dev_vec(ctx, logshape)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] for k in ("mean", "var", "lpd", "lpd_sum")]
    if upper is None and name != "bsc_weibull_predict_pass_interval":
        ctx.call(name, Xd, D, yd, od, B, D, Wd, pd, S, *args)
    else:
        ctx.call(name, Xd, D, yd, ud, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, upper, W, logshape, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, logshape, y, upper, o, v)
    bnd = ref.predict_bounds(X, W, logshape, y, upper, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("weibull interval %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


@pytest.mark.parametrize("B,D,S,offset", [(165, 12, 8, True), (1003, 256, 8, False), (325, 256, 64, True),
                                          (165, 12, 64, False)])
def test_predict_matches_the_reference(ctx, B, D, S, offset):
    X, y, upper, W, logshape, o, _ = ref.make_inputs(B, D, S, B + D + S, mode="offset" if offset else "none")
    assert min(_kinds(y, upper, None)) > 0
    got = _predict(ctx, X, y, upper, W, logshape, o)
    _assert_predict(got, X, y, upper, W, logshape, o)
    # upper == NULL: the bits of the predictive without it (every row then read as y says)
    a = _predict(ctx, X, y, None, W, logshape, o)
    b = _predict(ctx, X, y, None, W, logshape, o, name="bsc_weibull_predict_pass")
    for k in a:
        npt.assert_array_equal(a[k], b[k])
    npt.assert_array_equal(got["mean"], b["mean"])                      # the moments do not depend on the row's kind
    npt.assert_array_equal(got["var"], b["var"])


# ---- 5. the driver -----------------------------------------------------------------------------------------------------------

def _coarsened(B, D, seed, k=1.5, share=0.5, w=None, grid=0.5):
    """Weibull(k, scale e^{x . w + o}) durations, all events; a share of them known only to lie between two inspections
    ``grid`` apart (the first inspection at ``grid``: an event before it is left-censored).  Returns X, o, the exact
    times, and (time, upper) as the driver takes them, upper = inf where the time is exact."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.3 * rs.standard_normal(B)).astype(np.float32)
    w = rs.standard_normal(D) if w is None else w
    t = (np.exp(X.astype(np.float64) @ w + o) * rs.weibull(k, B)).astype(np.float32)
    t = np.maximum(t, np.float32(1e-6))
    coarse = rs.uniform(size=B) < share
    lo = (np.floor(t / grid) * grid).astype(np.float32)
    time = np.where(coarse, lo, t).astype(np.float32)
    upper = np.where(coarse, lo + np.float32(grid), np.inf).astype(np.float32)
    return X, o, t, time, upper, coarse


@pytest.mark.parametrize("covariance", ["diag", "full"])
def test_five_updates_track_the_reference_driver(ctx, covariance):
    from bayesic_amd.svi import WeibullReparamSVI
    from bayesic_amd.svi.glm_weibull import pack_censored
    import _glm_scalar_full_ref as fref
    S, B, D, seed, lr, prec, a0, b0 = 11, 1029, 256, 1234, 0.01, 2.0, 1.5, 0.5
    X, o, _, time, upper, coarse = _coarsened(B, D, 10)
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    y, u = pack_censored(time, None, upper)
    assert (u > 0).sum() > 100 and (u < 0).sum() > 10 and (u == 0).sum() > 100
    model = WeibullReparamSVI(X, time, upper=upper, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr,
                              prior_precision=prec, a0=a0, b0=b0, ctx=ctx, offset=o, weights=v, covariance=covariance)
    npt.assert_array_equal(model.y.cpu().numpy(), y)
    npt.assert_array_equal(model.upper.cpu().numpy(), u)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    full = covariance == "full"
    lam = fref.init_lam(D + 1) if full else ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    try:
        for t in range(1, 6):
            assert model.step() is None
            eps = ref.noise(D, S, seed, t - 1)
            W_r, lp_r = fref.draw(lam, eps) if full else ref.draw(lam, eps)
            ell, G, T = ref.data_pass(X, y, u, W_r, lp_r, o, v)
            size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(X, y, u, W_r, lp_r, o, v)[0], 10.0, prec, a0, b0,
                                       lam[fref.diag_slots(D + 1)] if full else lam[D + 1:])
            upd = fref.finish if full else ref.update
            lam, m1, m2, elbo, grad = upd(lam, m1, m2, t, eps, W_r, lp_r, ell, G, T, 10.0, prec, a0, b0, lr)
            ctx.sync()
            g = model.grad.cpu().numpy()
            e = abs(model.elbo.item() - elbo)
            print("%s t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g; lam err %.3g" % (
                covariance, t, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max(),
                np.abs(model.lam.cpu().numpy() - lam).max()))
            assert e <= 1e-6 * size, (e, size)
            assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert PASS in calls and PLAIN not in calls
    assert ("bsc_glm_scalar_fullrank_update" if full else "bsc_glm_weibull_update") in calls


def test_driver_predict_and_heldout_lpd_take_upper(ctx):
    from bayesic_amd.svi import WeibullReparamSVI
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi.glm_weibull import pack_censored
    B, D = 600, 8
    X, o, _, time, upper, _ = _coarsened(B, D, 12)
    m = WeibullReparamSVI(X, time, upper=upper, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    draws = mod.posterior_draws(m, 16)
    W, logshape = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    y, u = pack_censored(time, None, upper)
    out = m.predict(X, time, upper=upper, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, u, W, logshape, o)
    assert m.heldout_lpd(X, time, upper=upper, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    # the lpd of an interval row is the log of a probability, and the survival curve is what it was
    assert (got["lpd"][u != 0] <= 0).all()
    s = m.survival(X, np.maximum(time, np.float32(0.1)), offset=o, draws=draws).cpu().numpy()
    assert ((s >= 0) & (s <= 1)).all()
    with pytest.raises(ValueError, match="upper= needs time="):
        m.predict(X, upper=upper, offset=o)


# ---- 6. recovery ---------------------------------------------------------------------------------------------------------------

def test_interval_rows_recover_the_shape_that_midpoints_miss(ctx):
    """4000 rows at k = 1.5, D = 8, 300 full-batch updates.  Half of the events are known only to the inspection
    interval (0.5 wide, the scale being about 1; before the first inspection: left-censored).  Fitted once with those
    rows interval-censored and once with their midpoints taken as exact times: the interval fit's posterior mean of tau
    lands closer to log 1.5 than the midpoint fit's."""
    from bayesic_amd.svi import WeibullReparamSVI
    B, D, S, seed, steps, lr = 4000, 8, 8, 31, 300, 0.02
    w_true = np.array([0.8, -0.6, 0.4, 0.3, -0.2, 0.5, -0.4, 0.1])
    X, o, t, time, upper, coarse = _coarsened(B, D, 5, k=1.5, share=0.5, w=w_true)
    assert 0.45 < coarse.mean() < 0.55 and (time[coarse] == 0).any()
    mid = np.where(coarse, time + np.float32(0.25), t).astype(np.float32)
    fits = {}
    for name, kw in (("interval", dict(time=time, upper=upper)), ("midpoint", dict(time=mid))):
        m = WeibullReparamSVI(X, n_samples=S, seed=seed, lr=lr, ctx=ctx, offset=o, **kw)
        for _ in range(steps):
            m.step()
        ctx.sync()
        fits[name] = float(m.lam.cpu().numpy()[D])
    truth = math.log(1.5)
    print("tau: simulated %.4f, interval fit %.4f, midpoint fit %.4f" % (truth, fits["interval"], fits["midpoint"]))
    assert math.isfinite(fits["interval"]) and math.isfinite(fits["midpoint"])
    assert abs(fits["interval"] - truth) < abs(fits["midpoint"] - truth)


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
