"""GPU parity of the ordinal route (csrc/bsc_glm_ordinal.hip through the C ABI, svi/glm_ordinal.py, svi/predict.py)
against the float64 restatement in tests/_glm_ordinal_ref.py.

Tolerances are tests/test_glm_weibull_gpu.py's construction with this likelihood's bound quantities, which the reference
computes from the sizes of the terms and the conditioning of a = c_{y-1} - eta, b = c_y - eta on their rounded inputs
(tests/_glm_ordinal_ref.py's docstring):
 * ell and every entry of G (the K - 1 columns of d ell / d theta included): |dev - ref| <= EPS * bound quantity,
   EPS = 2e-5; dropped rows are left out;
 * several updates against the reference driver: gradient 1e-4 * max|grad|, lam atol 2e-4 over 20 steps, the ELBO within
   1e-6 of the sum of the absolute values of its terms -- tests/test_glm_weibull_gpu.py's three;
 * the predictive: tests/_glm_ordinal_ref.predict_bounds; every row of prob adds up to 1 within K float32 ulps of 1.
The log-gaps stay inside the accuracy envelope [-3, 1.5] and |eta| <= 30.  A plain float32 evaluation of the pass's forms
stays below EPS / 20 of the bound quantities at these shapes (tests/test_glm_ordinal_cpu.py), which leaves a factor 20
for the device's reduction order and its fast logarithm; the measured ratios are printed.  Worst ratios of error to
tolerance on an MI355X (this file's own report, -s): ell 4.2e-4, G's weight columns 5.3e-4, G's theta columns 1.9e-3; the
driver's ELBO 3.4e-3 and gradient 3.3e-4 of theirs; the predictive's prob 7.4e-3, lpd 1.3e-2, lpd_sum 1.2e-3; the worst
row of prob is 0.94 ulps of 1 off (K >= 2 ulps allowed).

Shapes are the smallest that reach each route: (1003, 12) and (517, 200) the 8-row kernel, narrow and ragged;
(1003, 256) with y one int off 16-byte alignment the 8-row D == 256 kernel; (1029, 256) aligned the 16-row MFMA kernel
with a ragged last tile; two batches sized from the device's CU count so that every wave runs two tiles.  S in
{3, 8, 11} (11 = two launches, the second with dead draw slots), K in {2, 3, 5, 8}, offset and weights each null and each
set, the rows of weight 0 holding labels -1, K and 2^31 - 1, ldx > D, ldz > P, Z four bytes off 16-byte alignment (P is
in general odd: the draws' rows are not 16-byte aligned either way); sentinels of 1e30 behind o and v and in every padding
column of Z.  Behind y the guard holds label 1, not the bits of 1e30: those are a label outside [0, K), which the pass
skips, so a read past the end would go unseen -- a valid label with a weight of 1e30 beside it does not."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_obs_ref as obs
import _glm_ordinal_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30      # behind the end of o / v and in the padding of Z: a read there would wreck the sums
WORST = {}             # what: worst device error / tolerance seen in this run (printed by each check)
ULP1 = float(np.finfo(np.float32).eps)


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host float vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _dev_labels(ctx, y, shift=False, guard=16):
    """The labels on the device with valid labels behind their end (module docstring)."""
    if y is None:
        return None
    buf = np.concatenate([[1] if shift else [], y, np.full(guard, 1)]).astype(np.int32)
    t = ctx.to_device(buf, torch.int32)
    return t[1:] if shift else t


def _dev_draws(ctx, Z, ldz=None, shift=False):
    """Z [S, P] on the device as [S, ldz] with sentinels in the padding columns; ``shift``: four bytes into its buffer."""
    S, P = Z.shape
    ldz = ldz or P
    buf = np.full(S * ldz + 1, SENTINEL, np.float32)
    view = buf[1:] if shift else buf[:-1]
    view.reshape(S, ldz)[:, :P] = Z
    t = ctx.to_device(buf)
    return (t[1:] if shift else t[:-1]), ldz


def _dev_X(ctx, X, ld=None):
    if ld is None:
        return ctx.to_device(X), X.shape[1]
    buf = np.full((X.shape[0], ld), 7.0, np.float32)         # the padding must never be read as data
    buf[:, :X.shape[1]] = X
    return ctx.to_device(buf), ld


def _pass(ctx, X, y, Z, K, o=None, v=None, ld=None, ldz=None, shift=()):
    B, D = X.shape
    S, P = Z.shape[0], D + K - 1
    Xd, ldx = _dev_X(ctx, X, ld)
    Zd, ldz = _dev_draws(ctx, Z, ldz, "z" in shift)
    yd = _dev_labels(ctx, y, "y" in shift)
    od, vd = _dev_vec(ctx, o, "o" in shift), _dev_vec(ctx, v, "v" in shift)
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, P), torch.float64)
    ctx.call("bsc_glm_ordinal_data_pass", Xd, ldx, yd, od, vd, B, D, K, Zd, ldz, S, ell, G)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy()


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _check_inputs(X, y, Z, o, v, K):
    """The conditions make_inputs promises (tests/_glm_ordinal_ref.py)."""
    B, D = X.shape
    keep = np.ones(B, bool) if v is None else v > 0
    assert set(y[keep]) == set(range(K)), "every level occurs among the kept rows"
    W, theta = ref.split(Z, D, K)
    if K > 2:
        assert ref.GAP_LO <= theta[:, 1:].min() and theta[:, 1:].max() <= ref.GAP_HI
    assert np.abs(obs.logits(X, W, o)).max() <= ref.ETA_MAX
    if v is not None:
        assert 0 < (~keep).sum() <= 0.1 * B
        dead = set(y[~keep])
        assert dead >= {-1, K, 2 ** 31 - 1} and not (dead & set(range(K)))


def _assert_close(got, X, y, Z, K, o, v, what="", factor=1.0):
    want = ref.data_pass(X, y, Z, K, o, v)
    bnd = ref.bounds(X, y, Z, K, o, v)
    D = X.shape[1]
    parts = (("ell", got[0], want[0], bnd[0]), ("G[w]", got[1][:, :D], want[1][:, :D], bnd[1][:, :D]),
             ("G[theta]", got[1][:, D:], want[1][:, D:], bnd[1][:, D:]))
    ratios = []
    for name, g, w, b in parts:
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (factor * ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d K=%d: error / tolerance ell %.3g, G[w] %.3g, G[theta] %.3g" % (
        what, X.shape[0], D, Z.shape[0], K, *ratios))
    for r, (name, _, _, _) in zip(ratios, parts):
        assert r <= 1.0, (name, r)


def _check(ctx, X, y, Z, K, o, v, **kw):
    _check_inputs(X, y, Z, o, v, K)
    got = _pass(ctx, X, y, Z, K, o, v, **kw)
    _assert_close(got, X, y, Z, K, o, v)
    return got


# ---- 1. parity at every route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,K,mode,ld,pad,shift", [
    (1003, 12, 8, 5, "both", 16, 3, ()), (1003, 12, 3, 2, "none", None, 0, ("z",)),
    (1003, 12, 11, 8, "weights", None, 1, ()), (1003, 12, 8, 3, "offset", None, 0, ()),
    (517, 200, 11, 3, "offset", None, 0, ("z",)), (517, 200, 3, 8, "both", 208, 5, ()),
    (517, 200, 8, 2, "weights", None, 0, ()), (517, 200, 8, 5, "none", None, 2, ()),
    (1003, 256, 8, 5, "both", None, 0, ("y",)), (1003, 256, 11, 2, "none", None, 7, ("y", "z")),
    (1003, 256, 3, 8, "weights", 260, 0, ("y",)),
    (1029, 256, 8, 8, "both", None, 0, ()), (1029, 256, 11, 5, "weights", 260, 4, ("z",)),
    (1029, 256, 3, 3, "offset", None, 1, ()), (1029, 256, 8, 2, "none", None, 0, ())])
def test_pass_matches_the_reference(ctx, B, D, S, K, mode, ld, pad, shift):
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=B * 7 + D + S + K, mode=mode)
    _check(ctx, X, y, Z, K, o, v, ld=ld, ldz=D + K - 1 + pad, shift=shift)


# ---- 2. every wave runs more than one tile ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D,K", [(16, 256, 8), (8, 12, 5)])
def test_two_tiles_per_wave_keep_the_H_accumulators_and_the_table(ctx, cu, rows, D, K):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows: the cutpoint-gradient accumulators
    and the (draw, class) table have to survive the hand-over from one tile to the next."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, Z, o, v = ref.make_inputs(B, D, 8, K, seed=rows + D)
    _check(ctx, X, y, Z, K, o, v)


# ---- 3. the same bits run to run; dropped rows change no bit ----------------------------------------------------------------

def test_two_runs_are_bit_identical(ctx):
    for B, D, S, K, seed in ((1029, 256, 11, 5, 5), (517, 200, 8, 8, 6)):
        X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=seed)
        a = _pass(ctx, X, y, Z, K, o, v)
        b = _pass(ctx, X, y, Z, K, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


@pytest.mark.parametrize("B,D", [(1029, 256), (1003, 256), (517, 200)])
def test_dropped_rows_change_no_bit_whatever_they_hold(ctx, B, D):
    """The same batch at the same partition with its dropped rows in three states: weight 0 and a quiet content (label 0,
    offset 0); weight 0 and labels -1, K, 2^31 - 1 with an offset of 1e30; a positive weight with those labels and that
    offset -- dropped by the label alone.  Every bit of ell and G is the same."""
    S, K = 8, 5
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=B + D)
    dead = v == 0
    assert dead.any() and set(y[dead]) >= {-1, K, 2 ** 31 - 1}
    shift = ("y",) if B == 1003 else ()
    quiet_y, quiet_o = np.where(dead, 0, y).astype(np.int32), np.where(dead, 0.0, o).astype(np.float32)
    wild_o = np.where(dead, SENTINEL, o).astype(np.float32)
    live_v = np.where(dead, 2.0, v).astype(np.float32)
    base = _pass(ctx, X, quiet_y, Z, K, quiet_o, v, shift=shift)
    _assert_close(base, X, y, Z, K, o, v)
    for yy, oo, vv in ((y, wild_o, v), (y, wild_o, live_v)):
        got = _pass(ctx, X, yy, Z, K, oo, vv, shift=shift)
        for p, q in zip(base, got):
            npt.assert_array_equal(p, q)


# ---- 4. a known answer: two levels are the logistic pass ----------------------------------------------------------------------

@pytest.mark.parametrize("B,D,mode", [(1029, 256, "both"), (517, 200, "none"), (1003, 12, "offset")])
def test_two_levels_are_the_logistic_pass_on_the_flipped_labels(ctx, B, D, mode):
    """K = 2 with theta_0 = c on every draw: P(y = 0) = sigmoid(c - eta), so the model is the logistic one at the linear
    predictor c - eta with the labels flipped -- bsc_glm_data_pass_obs on -X with y' = 1 - y and the offset c - o.  ell
    and the weights' columns of G agree within twice the tolerance (both sides are device results; the gradient with
    respect to w picks up the sign of -X twice and so agrees as it stands), and G[:, D] = d ell / d c = -sum_n v_n r_ns."""
    S, K, c = 8, 2, np.float32(0.375)
    X, y, Z, o, v = ref.make_inputs(B, D, S, K, seed=B + D, mode=mode)
    Z[:, D] = c
    ell, G = _pass(ctx, X, y, Z, K, o, v)
    _assert_close((ell, G), X, y, Z, K, o, v)
    yf = (1.0 - y.astype(np.float64)).astype(np.float32)          # (dropped rows: any float)
    of = (c - (np.zeros(B, np.float32) if o is None else o)).astype(np.float32)
    W = np.ascontiguousarray(Z[:, :D])
    ell_l, G_l = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    ctx.call("bsc_glm_data_pass_obs", 0, ctx.to_device(-X), D, _dev_vec(ctx, yf), _dev_vec(ctx, of), _dev_vec(ctx, v), B,
             D, ctx.to_device(W), S, ell_l, G_l)
    ctx.sync()
    _assert_close((ell_l.cpu().numpy(), np.concatenate([G_l.cpu().numpy(), G[:, D:]], axis=1)), X, y, Z, K, o, v,
                  what="logistic twin", factor=2.0)
    b_ell, b_G = ref.bounds(X, y, Z, K, o, v)
    assert (np.abs(ell - ell_l.cpu().numpy()) <= 2.0 * ref.EPS * b_ell).all()
    assert (np.abs(G[:, :D] - G_l.cpu().numpy()) <= 2.0 * ref.EPS * b_G[:, :D]).all()
    r_sum = ref._terms(X, y, Z, K, o, v)["r"].sum(axis=0)
    assert (np.abs(G[:, D] + r_sum) <= ref.EPS * b_G[:, D]).all()


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------

def _batch(B, D, K, seed):
    X, y, _, o, v = ref.make_inputs(B, D, 1, K, seed)
    y = np.where(v > 0, y, 0).astype(np.int32)            # the driver checks the labels of every row
    return X, y, o, v


@pytest.mark.parametrize("covariance,B,D,K,S", [("diag", 1029, 256, 4, 11), ("full", 517, 12, 5, 8)])
def test_twenty_updates_track_the_reference_over_two_batches(ctx, covariance, B, D, K, S):
    from bayesic_amd.svi import OrdinalReparamSVI
    seed, lr, prec = 1234, 0.01, 2.0
    P = D + K - 1
    batches = [_batch(B, D, K, 10 + k) for k in range(2)]
    dev = [(ctx.to_device(X), ctx.to_device(y, torch.int32), ctx.to_device(o), ctx.to_device(v)) for X, y, o, v in batches]
    X0, y0, o0, v0 = dev[0]
    model = OrdinalReparamSVI(X0, y0, K, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, ctx=ctx,
                              offset=o0, weights=v0, covariance=covariance)
    lam = ref.init_lam(P, covariance)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    finish = "bsc_glm_fullrank_update" if covariance == "full" else "bsc_glm_update"
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 21):
            k = (t - 1) % 2
            Xk, yk, ok, vk = dev[k]
            model.set_batch(Xk, yk, offset=ok, weights=vk)
            assert model.step() is None
            Xh, yh, oh, vh = batches[k]
            Z_r = ref.draw(lam, ref.noise(P, S, seed, t - 1), covariance)
            rho = (lam[ref.full.diag_slots(P)] if covariance == "full" else lam[P:]).copy()
            lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, Xh, yh, K, S, seed, 10.0 * B, lr, prec, offset=oh,
                                               weights=vh, covariance=covariance)
            if t in (1, 2, 3, 10, 20):
                size = ref.elbo_terms_size(Z_r, ref.bounds(Xh, yh, Z_r, K, oh, vh)[0], 10.0, prec, rho)
                ctx.sync()
                g = model.grad.cpu().numpy()
                e = abs(model.elbo.item() - elbo)
                print("%s t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g; lam err %.3g" % (
                    covariance, t, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max(),
                    np.abs(model.lam.cpu().numpy() - lam).max()))
                _note("driver elbo", e / (1e-6 * size))
                _note("driver grad", np.abs(g - grad).max() / (1e-4 * np.abs(grad).max()))
                assert e <= 1e-6 * size, (e, size)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    ctx.sync()
    assert "bsc_glm_ordinal_data_pass" in calls and finish in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and c not in ("bsc_glm_ordinal_data_pass", finish)]
    p = model.params()
    m = lam[:P]
    npt.assert_allclose(p["cutpoints"], np.cumsum(np.concatenate([m[D:D + 1], np.exp(m[D + 1:])])), atol=1e-3)


def test_a_fit_on_simulated_data_beats_the_class_frequencies_on_fresh_rows(ctx):
    """4000 rows at five levels with separated cutpoints, full batch, the step count at which the float64 reference
    driver alone meets the same three checks (tests/test_glm_ordinal_cpu.py): the ELBO rises from the first step to the
    last, every draw's cutpoints are increasing, and the held-out log density on fresh rows beats the log-likelihood of
    the training class frequencies on those rows -- a baseline that comes from the data."""
    from bayesic_amd import svi
    from test_glm_ordinal_cpu import FIT
    K = 5
    X, y = ref.simulate(FIT["B"], 5)
    Xt, yt = ref.simulate(2000, 6)
    m = svi.OrdinalReparamSVI(X, y, K, n_samples=FIT["S"], seed=FIT["seed"], lr=FIT["lr"], ctx=ctx)
    D = m.D
    elbos = []
    for t in range(FIT["steps"]):
        m.step()
        if t in (0, FIT["steps"] - 1):
            ctx.sync()
            elbos.append(m.elbo.item())
        Zs = m.W.cpu().numpy().reshape(m.S, m.P) if t % 25 == 0 or t == FIT["steps"] - 1 else None
        if Zs is not None:
            assert (np.diff(ref.cutpoints(Zs[:, D:]), axis=1) > 0).all(), t
    assert elbos[1] > elbos[0], elbos
    score = svi.heldout_lpd(m, Xt, yt, n_samples=64)
    base = ref.frequency_baseline(y, yt, K)
    print("device fit: ELBO %.1f -> %.1f, held-out lpd %.4f against the class frequencies' %.4f; cutpoints %s" % (
        elbos[0], elbos[1], score, base, m.params()["cutpoints"]))
    assert score > base
    assert (np.diff(m.params()["cutpoints"]) > 0).all()


# ---- 6. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, Z, K, o, ldz=None, shift=(), want=("prob", "lpd", "lpd_sum")):
    B, D = X.shape
    S = Z.shape[0]
    Xd, ldx = _dev_X(ctx, X)
    Zd, ldz = _dev_draws(ctx, Z, ldz, "z" in shift)
    yd, od = _dev_labels(ctx, y, "y" in shift), _dev_vec(ctx, o, "o" in shift)
    out = {"prob": torch.full((B, K), -777.0, dtype=torch.float32, device=ctx.device),
           "lpd": torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device),
           "lpd_sum": torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)}
    args = [out[k] if k in want else None for k in ("prob", "lpd", "lpd_sum")]
    ctx.call("bsc_ordinal_predict_pass", Xd, ldx, yd, od, B, D, K, Zd, ldz, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, Z, K, o, v=None, keys=("prob", "lpd", "lpd_sum")):
    want = ref.predict(X, Z, K, y, o, v)
    bnd = ref.predict_bounds(X, Z, K, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("ordinal %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)
    rows = np.abs(got["prob"].astype(np.float64).sum(axis=1) - 1.0)
    _note("prob row sums", rows.max() / (K * ULP1))
    print("ordinal prob rows: worst |sum - 1| = %.3g ulps of 1 (K = %d allowed)" % (rows.max() / ULP1, K))
    assert (rows <= K * ULP1).all(), rows.max() / ULP1


def _predict_inputs(B, D, S, K, seed, offset=True):
    X, y, Z, o, _ = ref.make_inputs(B, D, S, K, seed, mode="offset")
    y = y.copy()
    y[3], y[B // 2] = -1, K                         # rows that score 0
    return X, y, Z, (o if offset else None)


@pytest.mark.parametrize("B,D,S,K,shift,offset,pad", [
    (37, 12, 5, 5, (), True, 0), (165, 12, 16, 2, ("o", "z"), False, 3), (53, 12, 40, 8, (), True, 1),
    (165, 12, 64, 3, ("y",), True, 0), (37, 256, 5, 8, ("o",), True, 0), (1003, 256, 16, 5, ("z",), False, 4),
    (325, 256, 40, 3, (), True, 0), (1003, 256, 64, 8, ("y", "o"), True, 2)])
def test_predict_matches_the_reference(ctx, B, D, S, K, shift, offset, pad):
    X, y, Z, o = _predict_inputs(B, D, S, K, B + D + S + K, offset)
    got = _predict(ctx, X, y, Z, K, o, ldz=D + K - 1 + pad, shift=shift)
    _assert_predict(got, X, y, Z, K, o)
    assert got["lpd"][3] == 0.0 and got["lpd"][B // 2] == 0.0       # a label outside [0, K) scores 0


def test_predict_without_y_gives_the_probabilities_alone(ctx):
    X, y, Z, o = _predict_inputs(165, 12, 16, 5, 9)
    full = _predict(ctx, X, y, Z, 5, o)
    got = _predict(ctx, X, None, Z, 5, o, want=("prob",))
    npt.assert_array_equal(got["prob"], full["prob"])
    assert (got["lpd"] == -777.0).all() and got["lpd_sum"][0] == -777.0
    got = _predict(ctx, X, y, Z, 5, o, want=("lpd_sum",))
    npt.assert_array_equal(got["lpd_sum"], full["lpd_sum"])
    assert (got["lpd"] == -777.0).all() and (got["prob"] == -777.0).all()


def test_driver_predict_heldout_lpd_and_posterior_draws(ctx):
    from bayesic_amd import svi
    from bayesic_amd.svi import predict as mod
    B, D, K = 600, 8, 5
    X, y, o, _ = _batch(B, D, K, 12)
    m = svi.OrdinalReparamSVI(X, y, K, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "ordinal"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    draws = mod.posterior_draws(m, 16)
    assert draws[1] is None and tuple(draws[0].shape) == (16, m.P) and draws[0].dtype == torch.float32
    Z = draws[0].cpu().numpy()
    npt.assert_array_equal(Z, ref.posterior_draws(m.lam.cpu().numpy(), m.P, 16, m.seed))        # Philox stream 2 ...
    train = ref.draw(m.lam.cpu().numpy(), ref.noise(m.P, 16, m.seed, 0))
    assert not np.isin(Z, train).any()                                                        # ... never stream 0's
    out = m.predict(X, y, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, Z, K, o)
    via = mod.predict(m, X, y, offset=o, draws=draws)
    for k in ("prob", "lpd", "lpd_sum"):
        npt.assert_array_equal(via[k].cpu().numpy(), got[k])
    assert m.heldout_lpd(X, y, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    assert svi.heldout_lpd(m, X, y, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    probs = m.predict(X, offset=o, draws=draws)
    assert set(probs) == {"prob"}
    npt.assert_array_equal(probs["prob"].cpu().numpy(), got["prob"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("prob", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, Z, K, o, v)
    score = svi.heldout_lpd(m, X, y, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    # a model fitted without an offset predicts without one
    m0 = svi.OrdinalReparamSVI(X, y, K, n_samples=8, seed=9, ctx=ctx)
    m0.step()
    d0 = mod.posterior_draws(m0, 40)
    g0 = {k: a.cpu().numpy() for k, a in m0.predict(X, y, draws=d0).items()}
    _assert_predict(g0, X, y, d0[0].cpu().numpy(), K, None)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_quantity_and_leave_the_outputs_alone(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, Z = ctx.zeros((9, 260)), ctx.zeros(12, torch.int32), ctx.zeros((65, 270))
    o, v = ctx.zeros(12), ctx.zeros(12)
    ell, G = ctx.zeros(65, f64) + 5.0, ctx.zeros((65, 270), f64) + 5.0
    prob = ctx.zeros((9, 8)) + 5.0

    def train(ldx, D, K, S, ldz=270):
        ctx.call("bsc_glm_ordinal_data_pass", X, ldx, y, o, v, 8, D, K, Z, ldz, S, ell, G)

    def predict(ldx, D, K, S, ldz=270):
        ctx.call("bsc_ordinal_predict_pass", X, ldx, y, o, 8, D, K, Z, ldz, S, prob, None, None)

    for fn, who, code in ((train, "bsc_glm_ordinal_data_pass", -1), (predict, "bsc_ordinal_predict_pass", -3)):
        for args, match in (((12, 10, 5, 8), "%s: D=10 must be a multiple of 4" % who),
                            ((260, 260, 5, 8), "%s: D=260 must be a multiple of 4 in" % who),
                            ((256, 256, 5, 65), "%s: S=65" % who),
                            ((10, 12, 5, 8), "%s: ldx=10" % who)):
            with pytest.raises(BayesicHipError, match=match) as err:
                fn(*args)
            assert "status %d:" % code in str(err.value), str(err.value)
        for K in (1, 9):
            with pytest.raises(BayesicHipError, match=r"%s: K=%d must be in \[2,8\]" % (who, K)) as err:
                fn(256, 256, K, 8)
            assert "status -1:" in str(err.value)
        with pytest.raises(BayesicHipError, match="%s: ldz=259" % who) as err:
            fn(256, 256, 5, 8, ldz=259)
        assert "status -1:" in str(err.value)
    with pytest.raises(BayesicHipError, match="bsc_ordinal_predict_pass: lpd and lpd_sum need y"):
        ctx.call("bsc_ordinal_predict_pass", X, 256, None, o, 8, 256, 5, Z, 270, 8, prob, o, None)
    with pytest.raises(BayesicHipError, match="bsc_ordinal_predict_pass: no output requested"):
        ctx.call("bsc_ordinal_predict_pass", X, 256, y, o, 8, 256, 5, Z, 270, 8, None, None, None)
    ctx.sync()
    assert (ell.cpu().numpy() == 5.0).all() and (G.cpu().numpy() == 5.0).all() and (prob.cpu().numpy() == 5.0).all()
    # B = 0 gives zeros
    ctx.call("bsc_glm_ordinal_data_pass", X, 256, y, o, v, 0, 256, 5, Z, 270, 8, ell, G)
    ctx.sync()
    assert (ell.cpu().numpy()[:8] == 0.0).all() and (G.cpu().numpy().ravel()[:8 * 260] == 0.0).all()


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
