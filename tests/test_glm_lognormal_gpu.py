"""GPU parity of the log-normal survival route (csrc/bsc_glm_lognormal.hip through the C ABI, svi/glm_lognormal.py,
svi/predict.py) against the float64 restatement in tests/_glm_lognormal_ref.py.

Tolerances are tests/test_glm_weibull_gpu.py's construction with this likelihood's bound quantities, which the reference
computes from the sizes of the terms and the conditioning of z = k (log t - l) on its rounded inputs
(tests/_glm_lognormal_ref.py's docstring):
 * ell, T and every entry of G: |dev - ref| <= EPS * bound quantity, EPS = 2e-5; rows of weight 0 are left out;
 * the finish on supplied statistics: the bits of bsc_glm_nb_update on the same arguments;
 * several updates against the reference driver: gradient 1e-4 * max|grad|, lam atol 2e-4 over 20 steps (1e-3 of the
   distance steps * lr that Adam can have moved a coordinate), the ELBO within 1e-6 of the sum of the absolute values of
   its terms -- tests/test_glm_weibull_gpu.py's three, for the reason given there (tests/test_glm_gamma_gpu.py);
 * the predictive: tests/_glm_lognormal_ref.predict_bounds.
tau stays inside the accuracy envelope [-1.5, 4] (include/bayesic_hip.h) and |z| at or below 60.  A plain float32
evaluation of the device's forms stays below 1e-6 of the bound quantities at these shapes
(tests/test_glm_lognormal_cpu.py), which leaves a factor 20 for the device's reduction order and its own special
function; the measured ratios are printed.

Shapes are the smallest that reach each route: (1003, 12) and (517, 200) the 8-row kernel, narrow and ragged;
(1003, 256) with y one float off 16-byte alignment the 8-row D == 256 kernel; (1029, 256) aligned the 16-row MFMA kernel
with a ragged last tile; two batches sized from the device's CU count so that every wave runs two tiles.  S in
{3, 8, 11} (11 = two launches, the second with dead draw slots), about 30 % of the rows censored (and one batch of all
events, one of all censored, one with z pinned at +-60 on censored rows: both tails of the special function), offset
and weights each null and each set, the rows of weight 0 holding y = 0 or NaN, ldx > D; sentinels of 1e30 behind y, o,
v and loginvscale."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_lognormal_ref as ref
import _glm_obs_ref as obs
import _glm_scalar_full_ref as full_ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30      # behind the end of y / o / v / loginvscale: a read past the end would wreck the sums
WORST = {}             # what: worst device error / (EPS * bound quantity) seen in this run (printed by each check)
PASS, FINISH, PREDICT = "bsc_glm_lognormal_data_pass", "bsc_glm_lognormal_update", "bsc_lognormal_predict_pass"


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, W, lis, o=None, v=None, ld=None, shift=()):
    B, D = X.shape
    S = W.shape[0]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    Wd = ctx.to_device(W)
    yd, od, vd = (_dev_vec(ctx, a, k in shift) for k, a in (("y", y), ("o", o), ("v", v)))
    pd = _dev_vec(ctx, lis, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    ctx.call(PASS, Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _assert_close(got, X, y, W, lis, o, v, what=""):
    want = ref.data_pass(X, y, W, lis, o, v)
    bnd = ref.bounds(X, y, W, lis, o, v)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d: error / tolerance ell %.3g, G %.3g, T %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)


def _check(ctx, X, y, W, lis, o, v, what="", **kw):
    assert ref.TAU_LO <= lis.min() and lis.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, W, lis, o, v, **kw)
    _assert_close(got, X, y, W, lis, o, v, what)
    return got


# ---- 1. parity at every route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,mode,ld,shift,censored", [
    (1003, 12, 8, "both", 16, (), 0.3), (1003, 12, 3, "none", None, (), 0.0), (1003, 12, 8, "weights", None, (), 1.0),
    (517, 200, 11, "offset", None, (), 0.3), (517, 200, 3, "both", 208, (), 0.3),
    (1003, 256, 8, "both", None, ("y",), 0.3), (1003, 256, 11, "none", None, ("y",), 0.3),
    (1029, 256, 8, "both", None, (), 0.3), (1029, 256, 11, "weights", 260, (), 0.3),
    (1029, 256, 3, "offset", None, (), 0.3)])
def test_pass_matches_the_reference(ctx, B, D, S, mode, ld, shift, censored):
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode, censored=censored)
    if v is not None:
        dead = y[v == 0]
        assert np.isnan(dead).any() and (dead == 0).any()       # rows of weight 0 hold what a kept row must not
    keep = np.ones(B, bool) if v is None else v > 0
    share = (y[keep] < 0).mean()
    assert share == censored if censored in (0.0, 1.0) else 0.2 < share < 0.4
    _check(ctx, X, y, W, lis, o, v, ld=ld, shift=shift)


@pytest.mark.parametrize("B,D,tau", [(1003, 12, 1.0), (1029, 256, ref.TAU_HI), (1003, 256, 0.0)])
def test_both_tails_of_the_special_function_with_z_pinned_at_plus_and_minus_60(ctx, B, D, tau):
    """Every row censored, z = +60 and -60 in turn at every draw: log Phi(-60) = -1805 with a hazard of 60, and
    log Phi(60) = -0 with a hazard of 0 -- neither a NaN nor an infinity, and the sums within their bounds.  (tau from 0
    up: below it t = e^{l +- 60 / k} leaves float32.)"""
    X, y, W, lis, o, v = ref.make_pinned(B, D, 8, B + D, tau=tau)
    z = math.exp(float(lis[0])) * (np.log(np.abs(y.astype(np.float64))) - obs.logits(X, W, o)[:, 0])
    assert (y < 0).all() and (np.abs(np.abs(z) - 60.0) < 0.05).all() and (z > 0).any() and (z < 0).any()
    ell, _, _ = _check(ctx, X, y, W, lis, o, v, what="z = +-60", shift=("y",) if B == 1003 and D == 256 else ())
    assert (ell < -1000.0).all()


# ---- 2. every wave runs more than one tile ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D", [(16, 256), (8, 12)])
def test_two_tiles_per_wave_keep_T_and_the_per_draw_scalars(ctx, cu, rows, D):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows: T and the draw's tau and k have to
    survive the hand-over from one tile to the next.  Every draw has its own tau, every row its own offset and weight."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, W, lis, o, v = ref.make_inputs(B, D, 8, seed=rows + D)
    _check(ctx, X, y, W, lis, o, v)


# ---- 3. the same bits run to run; the finish -------------------------------------------------------------------------------

def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (517, 200, 8, 6)):
        X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, lis, o, v)
        b = _pass(ctx, X, y, W, lis, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


@pytest.mark.parametrize("D,S", [(256, 8), (12, 11)])
def test_the_finish_returns_the_bits_of_the_negative_binomials(ctx, D, S):
    """bsc_glm_lognormal_update and bsc_glm_nb_update run one body: the same arguments give the same bits (and
    tests/test_glm_nb_gpu.py holds that body to the float64 reference)."""
    f64 = torch.float64
    P = D + 1
    rs = np.random.RandomState(D + S)
    seed, t = 77, 4
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, lis = ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(2 * P), 0.01 * rs.uniform(size=2 * P)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, _, _, elbo_r, grad_r = ref.update(lam, m1.copy(), m2.copy(), t, eps, W, lis, ell, G, T, scale, prec, a0, b0,
                                             lr)

    def run(name):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W=ctx.to_device(W.ravel()), lp=_dev_vec(ctx, lis),
                 W_n=ctx.zeros(S * D), lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64),
                 stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
        ctx.call(name, d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["lp"], D, S, scale, prec,
                 a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"], d["elbo"], d["grad"])
        ctx.sync()
        return {k: a.cpu().numpy() for k, a in d.items()}

    h, twin = run(FINISH), run("bsc_glm_nb_update")
    for k in ("elbo", "grad", "out", "m1", "m2", "W_n", "lp_n"):
        npt.assert_array_equal(h[k], twin[k], err_msg=k)
    npt.assert_allclose(h["elbo"][0], elbo_r, rtol=1e-9)              # and it is the reference's update, not zeros
    npt.assert_allclose(h["out"], lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(h["grad"], grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------

def _survival_data(B, D, seed, sigma=0.7, censored=0.3, w=None, intercept=False):
    """Durations LogNormal(x . w + o, sigma) and, independent of them given the row, censoring times LogNormal(x . w + o
    + c sigma, sigma) with c such that a share ``censored`` of the rows is cut (P(C < T) = Phi(-c / sqrt 2)): the
    observed time is the smaller of the two.  ``intercept``: the first column of X is 1."""
    from scipy.special import ndtri
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    if intercept:
        X[:, 0] = 1.0
    o = (0.5 * rs.standard_normal(B) + 0.5).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    w = rs.standard_normal(D) if w is None else w
    l = X.astype(np.float64) @ w + o
    t = np.exp(l + sigma * rs.standard_normal(B))
    c = np.exp(l + sigma * rs.standard_normal(B) - math.sqrt(2.0) * float(ndtri(censored)) * sigma)
    event = t <= c
    t = np.maximum(np.minimum(t, c), 1.0e-30).astype(np.float32)
    return X, t, event, o, v


def test_twenty_updates_track_the_reference_over_two_batches(ctx):
    from bayesic_amd.svi import LogNormalReparamSVI
    S, B, D, seed, lr, prec, a0, b0 = 11, 1029, 256, 1234, 0.01, 2.0, 1.5, 0.5
    batches = [_survival_data(B, D, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, t0, e0, o0, v0 = dev[0]
    model = LogNormalReparamSVI(X0, t0, e0, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec,
                                a0=a0, b0=b0, ctx=ctx, offset=o0, weights=v0)
    npt.assert_array_equal(model.y.cpu().numpy(), np.where(batches[0][2], batches[0][1], -batches[0][1]))
    assert 0.2 < 1.0 - batches[0][2].mean() < 0.4
    lam = ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 21):
            k = (t - 1) % 2
            Xk, tk, ek, ok, vk = dev[k]
            model.set_batch(Xk, tk, event=ek, offset=ok, weights=vk)
            assert model.step() is None
            Xh, th, eh, oh, vh = batches[k]
            yh = np.where(eh, th, -th).astype(np.float32)
            W_r, lp_r = ref.draw(lam, ref.noise(D, S, seed, t - 1))
            rho = lam[D + 1:].copy()
            lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, Xh, yh, S, seed, 10.0 * B, lr, prec, a0, b0, offset=oh,
                                               weights=vh)
            if t in (1, 2, 3, 10, 20):
                size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(Xh, yh, W_r, lp_r, oh, vh)[0], 10.0, prec, a0, b0, rho)
                ctx.sync()
                g = model.grad.cpu().numpy()
                e = abs(model.elbo.item() - elbo)
                print("t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g; lam err %.3g" % (
                    t, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max(),
                    np.abs(model.lam.cpu().numpy() - lam).max()))
                assert e <= 1e-6 * size, (e, size)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    ctx.sync()
    assert PASS in calls and FINISH in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_lognormal_" not in c]
    p = model.params()
    var = math.exp(2.0 * lam[2 * D + 1])
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(lam[D] + 0.5 * var), rtol=1e-3)
    npt.assert_allclose(p["sigma_mean"], math.exp(-lam[D] + 0.5 * var), rtol=1e-3)


def test_raw_pointers_take_the_signed_vector_as_it_is(ctx):
    from bayesic_amd.svi import LogNormalReparamSVI
    B, D = 325, 12
    X, t, event, o, v = _survival_data(B, D, 7)
    Xd, td, ed, od, vd = (ctx.to_device(a) for a in (X, t, event, o, v))
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        LogNormalReparamSVI(Xd, td - td[0], ctx=ctx)                    # one exact zero
    a = LogNormalReparamSVI(Xd, td, ed, ctx=ctx, offset=od, weights=vd)
    b = LogNormalReparamSVI(Xd, td, ctx=ctx)
    signed = ctx.to_device(np.where(event, t, -t).astype(np.float32))
    b.set_batch(Xd.data_ptr(), signed.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())
    a.step()
    b.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        a.predict(Xd, td)


def test_full_covariance_steps_against_the_full_reference(ctx):
    """covariance="full" at D = 12: bsc_glm_scalar_fullrank_update on this pass's statistics, ten updates next to the
    reference stepper of tests/_glm_scalar_full_ref.py with tests/_glm_lognormal_ref.data_pass, the three tolerances of
    the mean-field test above."""
    from bayesic_amd.svi import LogNormalReparamSVI
    B, D, S, seed, lr, prec, a0, b0, scale = 2000, 12, 8, 1234, 0.01, 2.0, 1.5, 0.5, 10.0
    P = D + 1
    X, t, event, o, v = _survival_data(B, D, 10)
    y = np.where(event, t, -t).astype(np.float32)
    model = LogNormalReparamSVI(X, t, event, n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec,
                                a0=a0, b0=b0, ctx=ctx, offset=o, weights=v, covariance="full")
    lam = full_ref.init_lam(P)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for step in range(1, 11):
            assert model.step() is None
            eps = ref.noise(D, S, seed, step - 1)
            W_r, lp_r = full_ref.draw(lam, eps)
            rho = lam[full_ref.diag_slots(P)]
            ell, G, T = ref.data_pass(X, y, W_r, lp_r, o, v)
            lam, m1, m2, elbo, grad = full_ref.finish(lam, m1, m2, step, eps, W_r, lp_r, ell, G, T, scale, prec, a0, b0,
                                                      lr)
            size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(X, y, W_r, lp_r, o, v)[0], scale, prec, a0, b0, rho)
            ctx.sync()
            g = model.grad.cpu().numpy()
            e = abs(model.elbo.item() - elbo)
            print("full t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g, lam err %.3g" % (
                step, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max(),
                np.abs(model.lam.cpu().numpy() - lam).max()))
            assert e <= 1e-6 * size, (e, size)
            assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert calls.count(PASS) == 10 and calls.count("bsc_glm_scalar_fullrank_update") == 10 and FINISH not in calls
    p = model.params()
    L = p["L"]
    assert L.shape == (P, P) and (np.triu(L, 1) == 0).all() and np.abs(np.tril(L, -1)).max() > 0
    npt.assert_allclose(model.covariance(), L @ L.T, rtol=1e-14)
    var = float((L[D] ** 2).sum())                                     # the marginal variance of tau
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(p["m"][D] + 0.5 * var), rtol=1e-14)
    npt.assert_allclose(p["sigma_mean"], math.exp(-p["m"][D] + 0.5 * var), rtol=1e-12)


# ---- 5. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, lis, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, lis, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call(PREDICT, Xd, D, yd, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, lis, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, lis, y, o, v)
    bnd = ref.predict_bounds(X, W, lis, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("lognormal %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    """make_inputs with the logits kept at |l| <= 3.5 (the predictive mean holds exp(l)); the durations are fitted again
    so that |z| <= 60 at the new logits."""
    X, y, W, lis, o, _ = ref.make_inputs(B, D, S, seed, mode="offset")
    peak = np.abs(obs.logits(X, W, o)).max()
    if peak > 3.5:
        W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    o = o if offset else None
    y = ref.refit(y, obs.logits(X, W, o), lis)
    assert (y > 0).any() and (y < 0).any()
    return X, y, W, lis, o


@pytest.mark.parametrize("B,D,S,shift,offset", [(37, 12, 8, False, True), (165, 12, 64, True, False),
                                                (37, 256, 8, True, True), (1003, 256, 64, False, False),
                                                (325, 256, 8, False, False), (165, 12, 64, False, True)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset):
    X, y, W, lis, o = _predict_inputs(B, D, S, B + D + S, offset)
    assert lis.min() == ref.TAU_LO and lis.max() == ref.TAU_HI
    got = _predict(ctx, X, y, W, lis, o, shift=shift)
    _assert_predict(got, X, y, W, lis, o)


def test_predict_without_y_gives_the_moments_alone(ctx):
    X, y, W, lis, o = _predict_inputs(165, 12, 8, 9)
    full = _predict(ctx, X, y, W, lis, o)
    B, D = X.shape
    mean, var = (torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for _ in range(2))
    ctx.call(PREDICT, ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W), _dev_vec(ctx, lis), 8, mean,
             var, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])
    npt.assert_array_equal(var.cpu().numpy(), full["var"])
    _assert_predict(dict(mean=mean.cpu().numpy(), var=var.cpu().numpy()), X, None, W, lis, o, keys=("mean", "var"))
    got = _predict(ctx, X, y, W, lis, o, want=("lpd_sum",))
    npt.assert_array_equal(got["lpd_sum"], full["lpd_sum"])
    assert (got["lpd"] == -777.0).all() and (got["mean"] == -777.0).all()


def test_driver_predict_heldout_lpd_and_survival(ctx):
    from bayesic_amd.svi import LogNormalReparamSVI
    from bayesic_amd.svi import predict as mod
    B, D = 600, 8
    X, t, event, o, _ = _survival_data(B, D, 12)
    m = LogNormalReparamSVI(X, t, event, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "lognormal"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, t, event)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the lognormal model takes offset="):
        mod.predict(m, X, None, exposure=np.ones(B, np.float32))
    with pytest.raises(ValueError, match="belongs to the Weibull model, not lognormal"):
        mod.predict(m, X, t, offset=o, upper=np.ones(B, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, t, offset=o, groups=np.zeros(B, np.int32))
    draws = mod.posterior_draws(m, 16)
    W, lis = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(lis, lp_r)
    y = np.where(event, t, -t).astype(np.float32)
    out = m.predict(X, t, event, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, W, lis, o)
    assert m.heldout_lpd(X, t, event, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    moments = m.predict(X, offset=o, draws=draws)
    assert set(moments) == {"mean", "var"}
    npt.assert_array_equal(moments["mean"].cpu().numpy(), got["mean"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, t, event, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, lis, o, v)
    score = m.heldout_lpd(X, t, event, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    # survival: exp of the lpd with every row censored at t_n, within that lpd's bound (d e^x = e^x dx, and one rounding)
    s = m.survival(X, t, offset=o, draws=draws)
    assert s.dtype == torch.float32 and tuple(s.shape) == (B,)
    s = s.cpu().numpy()
    s_ref = ref.survival(X, W, lis, t, o)
    tol = s_ref * ref.predict_bounds(X, W, lis, -t, o)["lpd"] + ref.EPS * s_ref + float(np.finfo(np.float32).tiny)
    _note("survival", np.max(np.abs(s - s_ref) / tol))
    assert (np.abs(s - s_ref) <= tol).all(), np.max(np.abs(s - s_ref) / tol)
    # in [0, 1] and non-increasing in t for a fixed row
    grid = np.exp(np.linspace(math.log(1e-3), math.log(200.0), 64)).astype(np.float32)
    Xrow = np.repeat(X[5:6], 64, axis=0)
    orow = np.repeat(o[5:6], 64)
    curve = m.survival(Xrow, grid, offset=orow, draws=draws).cpu().numpy()
    assert (curve >= 0.0).all() and (curve <= 1.0).all()
    assert (np.diff(curve) <= 0.0).all() and curve[0] > 0.99 and curve[-1] < 0.5
    # a model fitted without an offset predicts without one
    m0 = LogNormalReparamSVI(X, t, event, n_samples=8, seed=9, ctx=ctx)
    m0.step()
    d0 = mod.posterior_draws(m0, 40)
    g0 = {k: a.cpu().numpy() for k, a in m0.predict(X, t, event, draws=d0).items()}
    _assert_predict(g0, X, y, d0[0].cpu().numpy(), d0[1].cpu().numpy(), None)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_come_from_the_shared_checks_with_their_codes(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9) + 1.0, ctx.zeros((65, 260))
    o, v, lp = ctx.zeros(12), ctx.zeros(12), ctx.zeros(68)
    ell, G, T = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros(65, f64)
    out = ctx.zeros(9)

    def train(ldx, D, S, pa=lp):
        ctx.call(PASS, X, ldx, y, o, v, 8, D, W, pa, S, ell, G, T)

    def predict(ldx, D, S, pa=lp):
        ctx.call(PREDICT, X, ldx, y, o, 8, D, W, pa, S, out, None, None, None)

    # the training pass refuses with bsc_glm_nb_data_pass's checks (invalid argument), the predictive with
    # bsc_nb_predict_pass's (unsupported)
    for fn, who, code in ((train, PASS, -1), (predict, PREDICT, -3)):
        for args, match in (((12, 10, 8), "%s: D=10 must be a multiple of 4" % who),
                            ((260, 260, 8), "%s: D=260 must be a multiple of 4 in" % who),
                            ((256, 256, 65), "%s: S=65" % who)):
            with pytest.raises(BayesicHipError, match=match) as err:
                fn(*args)
            assert "status %d:" % code in str(err.value), str(err.value)
        with pytest.raises(BayesicHipError, match="%s: loginvscale is null" % who) as err:
            fn(256, 256, 8, pa=None)
        assert "status -1:" in str(err.value)
    ctx.sync()


# ---- 7. recovery ------------------------------------------------------------------------------------------------------------

def _reference_fit(X, y, o, S, seed, steps, lr, prec, a0, b0):
    lam = ref.init_lam(X.shape[1])
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, steps + 1):
        lam, m1, m2, _, _ = ref.step(lam, m1, m2, t, X, y, S, seed, float(X.shape[0]), lr, prec, a0, b0, offset=o)
    return lam


def test_recovery_follows_the_reference_driver_and_ignoring_the_censoring_shrinks_scale_and_intercept(ctx):
    """3000 rows at sigma = 0.5 with an intercept column, about 30 % censored by independent censoring times, 300
    full-batch updates from one seed on the device and in the float64 reference driver.  The fitted w and tau are held to
    the reference's within steps * lr * 1e-3 -- tests/test_glm_weibull_gpu.py's rule: an Adam step moves a coordinate by
    about lr at most, and the float32 pass's gradient error (held to 1e-4 of the largest entry above) is allowed to bend
    a thousandth of that path.  The tolerance, 6e-3, is a fraction of the posterior standard deviations (printed), so the
    comparison is with the reference run, not with a band around the truth.  Then the same durations with the censored
    rows passed as events: every cut duration is shorter than the event it hides and the upper tail is clipped, so
    sigma_mean and the intercept both move DOWN, in the reference and on the device."""
    from bayesic_amd.svi import LogNormalReparamSVI
    B, D, S, seed, steps, lr, prec, a0, b0 = 3000, 8, 8, 31, 300, 0.02, 1.0, 1.0, 0.1
    w_true = np.array([0.8, -0.6, 0.4, 0.3, -0.2, 0.5, -0.4, 0.1])
    X, t, event, o, _ = _survival_data(B, D, 5, sigma=0.5, censored=0.3, w=w_true, intercept=True)
    y = np.where(event, t, -t).astype(np.float32)
    assert 0.25 < 1.0 - event.mean() < 0.35
    tol = steps * lr * 1e-3
    fits = {}
    for name, ev, yy in (("censored", event, y), ("naive", None, t)):
        m = LogNormalReparamSVI(X, t, ev, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0, b0=b0, ctx=ctx,
                                offset=o)
        for _ in range(steps):
            m.step()
        ctx.sync()
        lam_d, lam_r = m.lam.cpu().numpy(), _reference_fit(X, yy, o, S, seed, steps, lr, prec, a0, b0)
        err = np.abs(lam_d[:D + 1] - lam_r[:D + 1]).max()
        print("%s: tau dev %.5f ref %.5f, max |m dev - m ref| %.3g (tolerance %.3g), posterior sd %.3g .. %.3g" % (
            name, lam_d[D], lam_r[D], err, tol, np.exp(lam_r[D + 1:]).min(), np.exp(lam_r[D + 1:]).max()))
        _note("recovery " + name, err / tol)
        assert err <= tol, (name, err)
        sigma_ref = math.exp(-lam_r[D] + 0.5 * math.exp(2.0 * lam_r[2 * D + 1]))
        fits[name] = (m.params()["sigma_mean"], lam_d[0], sigma_ref, lam_r[0])
    (sd_c, b_c, sr_c, br_c), (sd_n, b_n, sr_n, br_n) = fits["censored"], fits["naive"]
    print("sigma_mean censored %.4f naive %.4f; intercept censored %.4f naive %.4f" % (sd_c, sd_n, b_c, b_n))
    assert abs(sr_c - 0.5) < 0.05 and abs(br_c - 0.8) < 0.1          # the reference run itself found scale and intercept
    assert sr_n < sr_c - 10.0 * tol and br_n < br_c - 10.0 * tol     # the naive fit is clearly below in both ...
    assert sd_n < sd_c and b_n < b_c                                 # ... and the device moved the same way


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
