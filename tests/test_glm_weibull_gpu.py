"""GPU parity of the Weibull survival route (csrc/bsc_glm_weibull.hip through the C ABI, svi/glm_weibull.py,
svi/predict.py) against the float64 restatement in tests/_glm_weibull_ref.py.

Tolerances are tests/test_glm_gamma_gpu.py's construction with this likelihood's bound quantities, which the reference
computes from the sizes of the terms and the conditioning of z = k (log t - l) on its rounded inputs
(tests/_glm_weibull_ref.py's docstring):
 * ell, T and every entry of G: |dev - ref| <= EPS * bound quantity, EPS = 2e-5; rows of weight 0 are left out;
 * the finish on supplied statistics: the bits of bsc_glm_nb_update on the same arguments;
 * several updates against the reference driver: gradient 1e-4 * max|grad|, lam atol 2e-4 over 20 steps (1e-3 of the
   distance steps * lr that Adam can have moved a coordinate), the ELBO within 1e-6 of the sum of the absolute values of
   its terms -- tests/test_glm_gamma_gpu.py's three, for the reason given there;
 * the predictive: tests/_glm_weibull_ref.predict_bounds.
tau stays inside the accuracy envelope [-2, 4] (include/bayesic_hip.h) and z below 80: the link is not clamped.  A
plain float32 evaluation of the same formulas stays below 1e-6 of the bound quantities at these shapes
(tests/test_glm_weibull_cpu.py), which leaves a factor 20 for the device's reduction order; the measured ratios are
printed.

Shapes are the smallest that reach each route: (1003, 12) and (517, 200) the 8-row kernel, narrow and ragged;
(1003, 256) with y one float off 16-byte alignment the 8-row D == 256 kernel; (1029, 256) aligned the 16-row MFMA kernel
with a ragged last tile; two batches sized from the device's CU count so that every wave runs two tiles.  S in
{3, 8, 11} (11 = two launches, the second with dead draw slots), about 30 % of the rows censored (and one batch of all
events, one of all censored), offset and weights each null and each set, the rows of weight 0 holding y = 0 or NaN,
ldx > D; sentinels of 1e30 behind y, o, v and logshape."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_gamma_ref as gref
import _glm_obs_ref as obs
import _glm_weibull_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30      # behind the end of y / o / v / logshape: a read past the end would wreck the sums
WORST = {}             # what: worst device error / (EPS * bound quantity) seen in this run (printed by each check)


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, W, logshape, o=None, v=None, ld=None, shift=(), name="bsc_glm_weibull_data_pass"):
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
    pd = _dev_vec(ctx, logshape, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    ctx.call(name, Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _assert_close(got, X, y, W, logshape, o, v, what=""):
    want = ref.data_pass(X, y, W, logshape, o, v)
    bnd = ref.bounds(X, y, W, logshape, o, v)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d: error / tolerance ell %.3g, G %.3g, T %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)


def _check(ctx, X, y, W, logshape, o, v, **kw):
    assert ref.TAU_LO <= logshape.min() and logshape.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, W, logshape, o, v, **kw)
    _assert_close(got, X, y, W, logshape, o, v)
    return got


# ---- 1. parity at every route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,mode,ld,shift,censored", [
    (1003, 12, 8, "both", 16, (), 0.3), (1003, 12, 3, "none", None, (), 0.0), (1003, 12, 8, "weights", None, (), 1.0),
    (517, 200, 11, "offset", None, (), 0.3), (517, 200, 3, "both", 208, (), 0.3),
    (1003, 256, 8, "both", None, ("y",), 0.3), (1003, 256, 11, "none", None, ("y",), 0.3),
    (1029, 256, 8, "both", None, (), 0.3), (1029, 256, 11, "weights", 260, (), 0.3),
    (1029, 256, 3, "offset", None, (), 0.3)])
def test_pass_matches_the_reference(ctx, B, D, S, mode, ld, shift, censored):
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode, censored=censored)
    if v is not None:
        dead = y[v == 0]
        assert np.isnan(dead).any() and (dead == 0).any()       # rows of weight 0 hold what a kept row must not
    keep = np.ones(B, bool) if v is None else v > 0
    share = (y[keep] < 0).mean()
    assert share == censored if censored in (0.0, 1.0) else 0.2 < share < 0.4
    _check(ctx, X, y, W, logshape, o, v, ld=ld, shift=shift)


# ---- 2. every wave runs more than one tile ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D", [(16, 256), (8, 12)])
def test_two_tiles_per_wave_keep_T_and_the_per_draw_scalars(ctx, cu, rows, D):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows: T and the draw's tau and k have to
    survive the hand-over from one tile to the next.  Every draw has its own tau, every row its own offset and weight."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, W, logshape, o, v = ref.make_inputs(B, D, 8, seed=rows + D)
    _check(ctx, X, y, W, logshape, o, v)


# ---- 3. the same bits run to run; the Gamma pass at unit shape; the finish ------------------------------------------------

def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (517, 200, 8, 6)):
        X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, logshape, o, v)
        b = _pass(ctx, X, y, W, logshape, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


@pytest.mark.parametrize("B,D", [(1029, 256), (517, 200)])
def test_at_unit_shape_with_every_row_an_event_ell_and_G_are_the_gamma_passes(ctx, B, D):
    """tau = 0, every row an event: the two models coincide in ell and G (not in T).  The two device results differ by at
    most the sum of their two tolerances: EPS times the two bound quantities for ell, and for G this file's EPS * b_G
    plus tests/test_glm_gamma_gpu.py's 1e-4 * max|G|."""
    S = 8
    X, y, W, _, o, v = ref.make_inputs(B, D, S, seed=B + D, censored=0.0, tau=0.0)
    y = np.where(v > 0, y, 1.0).astype(np.float32)                  # the Gamma pass's dropped rows may hold anything too
    tau = np.zeros(S, np.float32)
    ell_w, G_w, _ = _pass(ctx, X, y, W, tau, o, v)
    ell_g, G_g, _ = _pass(ctx, X, y, W, tau, o, v, name="bsc_glm_gamma_data_pass")
    b_ell, b_G, _ = ref.bounds(X, y, W, tau, o, v)
    g_ell, _ = gref.bounds(X, y, W, tau, o, v)
    e_ell = np.abs(ell_w - ell_g) / (ref.EPS * (b_ell + g_ell))
    e_G = np.abs(G_w - G_g) / (ref.EPS * b_G + 1e-4 * np.abs(G_g).max())
    print("weibull against gamma at tau = 0: ell %.3g, G %.3g of the summed tolerances" % (e_ell.max(), e_G.max()))
    assert e_ell.max() <= 1.0 and e_G.max() <= 1.0


@pytest.mark.parametrize("D,S", [(256, 8), (12, 11)])
def test_the_finish_returns_the_bits_of_the_negative_binomials(ctx, D, S):
    """bsc_glm_weibull_update and bsc_glm_nb_update run one body: the same arguments give the same bits (and
    tests/test_glm_nb_gpu.py holds that body to the float64 reference)."""
    f64 = torch.float64
    P = D + 1
    rs = np.random.RandomState(D + S)
    seed, t = 77, 4
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, logshape = ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(2 * P), 0.01 * rs.uniform(size=2 * P)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, _, _, elbo_r, grad_r = ref.update(lam, m1.copy(), m2.copy(), t, eps, W, logshape, ell, G, T, scale, prec, a0,
                                             b0, lr)

    def run(name):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W=ctx.to_device(W.ravel()), lp=_dev_vec(ctx, logshape),
                 W_n=ctx.zeros(S * D), lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64),
                 stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
        ctx.call(name, d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["lp"], D, S, scale, prec,
                 a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"], d["elbo"], d["grad"])
        ctx.sync()
        return {k: a.cpu().numpy() for k, a in d.items()}

    h, twin = run("bsc_glm_weibull_update"), run("bsc_glm_nb_update")
    for k in ("elbo", "grad", "out", "m1", "m2", "W_n", "lp_n"):
        npt.assert_array_equal(h[k], twin[k], err_msg=k)
    npt.assert_allclose(h["elbo"][0], elbo_r, rtol=1e-9)              # and it is the reference's update, not zeros
    npt.assert_allclose(h["out"], lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(h["grad"], grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())


# ---- 4. the driver ----------------------------------------------------------------------------------------------------------

def _survival_data(B, D, seed, k=1.5, censored=0.3, w=None):
    """Durations Weibull(k, scale e^{x . w + o}), a share ``censored`` of them cut at a uniform fraction."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.5 * rs.standard_normal(B) + 0.5).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    w = rs.standard_normal(D) if w is None else w
    t = np.exp(X.astype(np.float64) @ w + o) * rs.weibull(k, B)
    event = rs.uniform(size=B) >= censored
    t = np.maximum(np.where(event, t, t * rs.uniform(0.1, 1.0, B)), 1.0e-30).astype(np.float32)
    return X, t, event, o, v


def test_twenty_updates_track_the_reference_over_two_batches(ctx):
    from bayesic_amd.svi import WeibullReparamSVI
    S, B, D, seed, lr, prec, a0, b0 = 11, 1029, 256, 1234, 0.01, 2.0, 1.5, 0.5
    batches = [_survival_data(B, D, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, t0, e0, o0, v0 = dev[0]
    model = WeibullReparamSVI(X0, t0, e0, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0,
                              b0=b0, ctx=ctx, offset=o0, weights=v0)
    npt.assert_array_equal(model.y.cpu().numpy(), np.where(batches[0][2], batches[0][1], -batches[0][1]))
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
    assert "bsc_glm_weibull_data_pass" in calls and "bsc_glm_weibull_update" in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_weibull_" not in c]
    p = model.params()
    npt.assert_allclose(p["shape_mean"], math.exp(lam[D] + 0.5 * math.exp(2.0 * lam[2 * D + 1])), rtol=1e-3)


def test_raw_pointers_take_the_signed_vector_as_it_is(ctx):
    from bayesic_amd.svi import WeibullReparamSVI
    B, D = 325, 12
    X, t, event, o, v = _survival_data(B, D, 7)
    Xd, td, ed, od, vd = (ctx.to_device(a) for a in (X, t, event, o, v))
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        WeibullReparamSVI(Xd, td - td[0], ctx=ctx)                      # one exact zero
    a = WeibullReparamSVI(Xd, td, ed, ctx=ctx, offset=od, weights=vd)
    b = WeibullReparamSVI(Xd, td, ctx=ctx)
    signed = ctx.to_device(np.where(event, t, -t).astype(np.float32))
    b.set_batch(Xd.data_ptr(), signed.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())
    a.step()
    b.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        a.predict(Xd, td)


# ---- 5. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, logshape, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, logshape, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call("bsc_weibull_predict_pass", Xd, D, yd, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, logshape, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, logshape, y, o, v)
    bnd = ref.predict_bounds(X, W, logshape, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("weibull %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    """make_inputs with the logits kept at |l| <= 3.5 (the predictive mean holds exp(l)); the durations are scaled again
    so that z <= 60 at the new logits."""
    X, y, W, logshape, o, _ = ref.make_inputs(B, D, S, seed, mode="offset")
    peak = np.abs(obs.logits(X, W, o)).max()
    if peak > 3.5:
        W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    o = o if offset else None
    k = np.exp(logshape.astype(np.float64))[None, :]
    over = (np.log(np.abs(y.astype(np.float64)))[:, None] - obs.logits(X, W, o) - 60.0 / k).max()
    y = (y * math.exp(-max(over, 0.0) - 1e-3)).astype(np.float32)
    assert (y > 0).any() and (y < 0).any()
    return X, y, W, logshape, o


@pytest.mark.parametrize("B,D,S,shift,offset", [(37, 12, 5, False, True), (165, 12, 16, True, False),
                                                (53, 12, 40, False, True), (165, 12, 64, False, True),
                                                (37, 256, 5, True, True), (1003, 256, 16, False, False),
                                                (325, 256, 40, False, True), (1003, 256, 64, True, True)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset):
    X, y, W, logshape, o = _predict_inputs(B, D, S, B + D + S, offset)
    got = _predict(ctx, X, y, W, logshape, o, shift=shift)
    _assert_predict(got, X, y, W, logshape, o)


def test_predict_without_y_gives_the_moments_alone(ctx):
    X, y, W, logshape, o = _predict_inputs(165, 12, 16, 9)
    full = _predict(ctx, X, y, W, logshape, o)
    B, D = X.shape
    mean, var = (torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for _ in range(2))
    ctx.call("bsc_weibull_predict_pass", ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W),
             _dev_vec(ctx, logshape), 16, mean, var, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])
    npt.assert_array_equal(var.cpu().numpy(), full["var"])
    got = _predict(ctx, X, y, W, logshape, o, want=("lpd_sum",))
    npt.assert_array_equal(got["lpd_sum"], full["lpd_sum"])
    assert (got["lpd"] == -777.0).all() and (got["mean"] == -777.0).all()


def test_driver_predict_heldout_lpd_and_survival(ctx):
    from bayesic_amd.svi import WeibullReparamSVI
    from bayesic_amd.svi import predict as mod
    B, D = 600, 8
    X, t, event, o, _ = _survival_data(B, D, 12)
    m = WeibullReparamSVI(X, t, event, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "weibull"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, t, event)
    draws = mod.posterior_draws(m, 16)
    W, logshape = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(logshape, lp_r)
    y = np.where(event, t, -t).astype(np.float32)
    out = m.predict(X, t, event, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, W, logshape, o)
    assert m.heldout_lpd(X, t, event, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    moments = m.predict(X, offset=o, draws=draws)
    assert set(moments) == {"mean", "var"}
    npt.assert_array_equal(moments["mean"].cpu().numpy(), got["mean"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, t, event, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, logshape, o, v)
    score = m.heldout_lpd(X, t, event, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    # survival: exp of the lpd with every row censored at t_n, within that lpd's bound (d e^x = e^x dx, and one rounding)
    s = m.survival(X, t, offset=o, draws=draws)
    assert s.dtype == torch.float32 and tuple(s.shape) == (B,)
    s = s.cpu().numpy()
    s_ref = ref.survival(X, W, logshape, t, o)
    tol = s_ref * ref.predict_bounds(X, W, logshape, -t, o)["lpd"] + ref.EPS * s_ref + float(np.finfo(np.float32).tiny)
    _note("survival", np.max(np.abs(s - s_ref) / tol))
    assert (np.abs(s - s_ref) <= tol).all(), np.max(np.abs(s - s_ref) / tol)
    # in [0, 1] and non-increasing in t for a fixed row
    grid = np.exp(np.linspace(math.log(1e-3), math.log(50.0), 64)).astype(np.float32)
    Xrow = np.repeat(X[5:6], 64, axis=0)
    orow = np.repeat(o[5:6], 64)
    curve = m.survival(Xrow, grid, offset=orow, draws=draws).cpu().numpy()
    assert (curve >= 0.0).all() and (curve <= 1.0).all()
    assert (np.diff(curve) <= 0.0).all() and curve[0] > 0.99 and curve[-1] < 0.5
    # a model fitted without an offset predicts without one
    m0 = WeibullReparamSVI(X, t, event, n_samples=8, seed=9, ctx=ctx)
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
        ctx.call("bsc_glm_weibull_data_pass", X, ldx, y, o, v, 8, D, W, pa, S, ell, G, T)

    def predict(ldx, D, S, pa=lp):
        ctx.call("bsc_weibull_predict_pass", X, ldx, y, o, 8, D, W, pa, S, out, None, None, None)

    # the training pass refuses with bsc_glm_nb_data_pass's checks (invalid argument), the predictive with
    # bsc_nb_predict_pass's (unsupported)
    for fn, who, code in ((train, "bsc_glm_weibull_data_pass", -1), (predict, "bsc_weibull_predict_pass", -3)):
        for args, match in (((12, 10, 8), "%s: D=10 must be a multiple of 4" % who),
                            ((260, 260, 8), "%s: D=260 must be a multiple of 4 in" % who),
                            ((256, 256, 65), "%s: S=65" % who)):
            with pytest.raises(BayesicHipError, match=match) as err:
                fn(*args)
            assert "status %d:" % code in str(err.value), str(err.value)
        with pytest.raises(BayesicHipError, match="%s: logshape is null" % who) as err:
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


def test_recovery_follows_the_reference_driver_and_censoring_moves_the_shape_its_way(ctx):
    """4000 rows at k = 1.5, about 30 % censored, 300 full-batch updates from one seed on the device and in the float64
    reference driver.  The fitted w and tau are held to the reference's within steps * lr * 1e-3 -- the rule behind
    tests/test_glm_gamma_gpu.py's 2e-4 over 20 steps at lr = 0.01: an Adam step moves a coordinate by about lr at most,
    and the float32 pass's gradient error (held to 1e-4 of the largest entry above) is allowed to bend a thousandth of
    that path.  The tolerance, 6e-3, is a fraction of the posterior standard deviations (printed), so the comparison
    is with the reference run, not with a band around the truth.  Then the same durations with the censored rows passed
    as events: tau moves away from the censored fit in the direction the reference's own naive fit moves."""
    from bayesic_amd.svi import WeibullReparamSVI
    B, D, S, seed, steps, lr, prec, a0, b0 = 4000, 8, 8, 31, 300, 0.02, 1.0, 1.0, 0.1
    w_true = np.array([0.8, -0.6, 0.4, 0.3, -0.2, 0.5, -0.4, 0.1])
    X, t, event, o, _ = _survival_data(B, D, 5, k=1.5, censored=0.3, w=w_true)
    y = np.where(event, t, -t).astype(np.float32)
    assert 0.25 < 1.0 - event.mean() < 0.35
    tol = steps * lr * 1e-3
    fits = {}
    for name, ev, yy in (("censored", event, y), ("naive", None, t)):
        m = WeibullReparamSVI(X, t, ev, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0, b0=b0, ctx=ctx,
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
        fits[name] = (lam_d, lam_r)
    (cd, cr), (nd, nr) = fits["censored"], fits["naive"]
    assert abs(cr[D] - math.log(1.5)) < 0.1                           # the reference run itself found the shape
    assert abs(nr[D] - cr[D]) > 10.0 * tol                            # the naive fit's shape is clearly elsewhere ...
    assert np.sign(nd[D] - cd[D]) == np.sign(nr[D] - cr[D])           # ... and the device moved the same way


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
