"""GPU parity of the Student-t route (csrc/bsc_glm_studentt.hip through the C ABI, svi/glm_studentt.py, svi/predict.py)
against the float64 restatement in tests/_glm_studentt_ref.py.

Tolerances are tests/test_glm_lognormal_gpu.py's construction with this likelihood's bound quantities, which the reference
computes from the sizes of the terms and the conditioning of z = k (y - l) on its rounded inputs
(tests/_glm_studentt_ref.py's docstring):
 * ell, T and every entry of G: |dev - ref| <= EPS * bound quantity, EPS = 2e-5; rows of weight 0 are left out;
 * the finish on supplied statistics: the bits of bsc_glm_nb_update on the same arguments;
 * five updates against the reference driver: tests/test_glm_lognormal_gpu.py's three -- gradient 1e-4 * max|grad|, lam
   atol 2e-4 (what that file holds its ten and its twenty updates to), the ELBO within 1e-6 of the sum of the absolute
   values of its terms;
 * the predictive: tests/_glm_studentt_ref.predict_bounds; var = +inf exactly at nu <= 2.
tau runs over [-3, 5], nu over {1, 2.5, 4, 30, 1e6}, |z| from 1e-3 to 1e4 at the first draw (and up to e^8 times that at
the others).  A plain float32 evaluation of the device's forms stays below 1e-6 of the bound quantities at these shapes
(tests/test_glm_studentt_cpu.py), which leaves a factor 20 for the device's reduction order; the measured ratios are
printed.

Shapes are the smallest that reach each route: (1003, 12) and (517, 200) the 8-row kernel, narrow and ragged, also with a
padded leading dimension; (1003, 256) with y one float off 16-byte alignment the 8-row D == 256 kernel; (1029, 256)
aligned the 16-row MFMA kernel with a ragged last tile; two batches sized from the device's CU count so that every wave
runs two tiles.  S in {3, 8, 11} (11 = two launches, the second with dead draw slots), offset and weights each null and
each set, the rows of weight 0 holding NaN, +inf, -inf and 0, ldx > D; sentinels of 1e30 behind y, o, v and
loginvscale."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_obs_ref as obs
import _glm_scalar_full_ref as full_ref
import _glm_studentt_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30      # behind the end of y / o / v / loginvscale: a read past the end would wreck the sums
WORST = {}             # what: worst device error / (EPS * bound quantity) seen in this run (printed by each check)
PASS, FINISH, PREDICT = "bsc_glm_studentt_data_pass", "bsc_glm_studentt_update", "bsc_studentt_predict_pass"


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _upload(ctx, X, y, W, lis, o=None, v=None, ld=None, shift=()):
    B, D = X.shape
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    yd, od, vd = (_dev_vec(ctx, a, k in shift) for k, a in (("y", y), ("o", o), ("v", v)))
    return Xd, (ld or D), yd, od, vd, ctx.to_device(W), _dev_vec(ctx, lis, "p" in shift)


def _run(ctx, dev, B, D, S, nu):
    Xd, ldx, yd, od, vd, Wd, pd = dev
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    ctx.call(PASS, Xd, ldx, yd, od, vd, B, D, Wd, pd, S, float(nu), ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _pass(ctx, X, y, W, lis, nu, o=None, v=None, ld=None, shift=()):
    return _run(ctx, _upload(ctx, X, y, W, lis, o, v, ld, shift), X.shape[0], X.shape[1], W.shape[0], nu)


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _assert_close(got, X, y, W, lis, nu, o, v, what=""):
    want = ref.data_pass(X, y, W, lis, nu, o, v)
    bnd = ref.bounds(X, y, W, lis, nu, o, v)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d nu=%g: error / tolerance ell %.3g, G %.3g, T %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], nu, *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)


def _check(ctx, X, y, W, lis, nu, o, v, what="", **kw):
    assert ref.TAU_LO <= lis.min() and lis.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, W, lis, nu, o, v, **kw)
    _assert_close(got, X, y, W, lis, nu, o, v, what)
    return got


# ---- 1. parity at every route, every nu of the list --------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,mode,ld,shift,nu", [
    (1003, 12, 8, "both", 16, (), 4.0), (1003, 12, 3, "none", None, (), 1.0), (1003, 12, 8, "weights", None, (), 30.0),
    (517, 200, 11, "offset", None, (), 2.5), (517, 200, 3, "both", 208, (), 1.0e6),
    (1003, 256, 8, "both", None, ("y",), 1.0), (1003, 256, 11, "none", None, ("y",), 1.0e6),
    (1029, 256, 8, "both", None, (), 4.0), (1029, 256, 11, "weights", 260, (), 2.5),
    (1029, 256, 3, "offset", None, (), 30.0), (1029, 256, 8, "none", None, (), 1.0e6)])
def test_pass_matches_the_reference(ctx, B, D, S, mode, ld, shift, nu):
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode)
    assert (o is None) == (mode in ("none", "weights")) and (v is None) == (mode in ("none", "offset"))
    if v is not None:
        dead = y[v == 0]            # rows of weight 0 hold what a kept row must not
        assert np.isnan(dead).any() and (dead == np.inf).any() and (dead == -np.inf).any() and (dead == 0).any()
    keep = np.ones(B, bool) if v is None else v > 0
    z0 = np.abs(math.exp(float(lis[0])) * (y.astype(np.float64) - obs.logits(X, W, o)[:, 0]))[keep]
    assert z0.min() < 2e-3 and z0.max() > 5e3              # from a row on the fit to a gross outlier
    _check(ctx, X, y, W, lis, nu, o, v, ld=ld, shift=shift)


def test_every_nu_of_the_list_is_covered_above():
    marks = [m for m in test_pass_matches_the_reference.pytestmark if m.name == "parametrize"]
    assert {case[-1] for case in marks[0].args[1]} == set(ref.NUS)


def test_nu_is_read_at_every_call(ctx):
    """Two consecutive calls on one context and the same device buffers, nu = 1 and then nu = 30 (and back): each matches
    its own reference, and the two differ by far more than the tolerance."""
    B, D, S = 1029, 256, 8
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=3)
    dev = _upload(ctx, X, y, W, lis, o, v)
    a = _run(ctx, dev, B, D, S, 1.0)
    b = _run(ctx, dev, B, D, S, 30.0)
    a2 = _run(ctx, dev, B, D, S, 1.0)
    _assert_close(a, X, y, W, lis, 1.0, o, v, "first call")
    _assert_close(b, X, y, W, lis, 30.0, o, v, "second call")
    for p, q in zip(a, a2):
        npt.assert_array_equal(p, q)
    bnd = ref.bounds(X, y, W, lis, 30.0, o, v)
    assert (np.abs(a[0] - b[0]) > 1e3 * ref.EPS * bnd[0]).all()


# ---- 2. every wave runs more than one tile ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D,nu", [(16, 256, 4.0), (8, 12, 1.0e6)])
def test_two_tiles_per_wave_keep_T_and_the_per_draw_scalars(ctx, cu, rows, D, nu):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows: T and the draw's four constants have
    to survive the hand-over from one tile to the next.  Every draw has its own tau, every row its own offset and
    weight."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, W, lis, o, v = ref.make_inputs(B, D, 8, seed=rows + D)
    _check(ctx, X, y, W, lis, nu, o, v)


# ---- 3. the same bits run to run; the finish -------------------------------------------------------------------------------

def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed, nu in ((1029, 256, 11, 5, 4.0), (517, 200, 8, 6, 1.0)):
        X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, lis, nu, o, v)
        b = _pass(ctx, X, y, W, lis, nu, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


@pytest.mark.parametrize("D,S", [(256, 8), (12, 11)])
def test_the_finish_returns_the_bits_of_the_negative_binomials(ctx, D, S):
    """bsc_glm_studentt_update and bsc_glm_nb_update run one body: the same arguments give the same bits (and
    tests/test_glm_nb_gpu.py holds that body to the float64 reference).  The finish never sees nu."""
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

def _robust_data(B, D, seed, sigma=0.5, outliers=0.1, blow=20.0, w=None, intercept=False):
    """y = x . w + o + sigma * noise, a share ``outliers`` of the rows with noise * ``blow``.  ``intercept``: the first
    column of X is 1."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    if intercept:
        X[:, 0] = 1.0
    o = (0.5 * rs.standard_normal(B) + 0.5).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    w = rs.standard_normal(D) if w is None else w
    noise = sigma * rs.standard_normal(B)
    bad = rs.uniform(size=B) < outliers
    y = (X.astype(np.float64) @ w + o + np.where(bad, blow * noise, noise)).astype(np.float32)
    return X, y, o, v, bad


STEPS, LR = 5, 0.01
LAM_ATOL = 2e-4                   # tests/test_glm_lognormal_gpu.py's, for its ten and its twenty updates alike


def _compare_step(ctx, model, lam, elbo, grad, size, tag):
    ctx.sync()
    g = model.grad.cpu().numpy()
    e = abs(model.elbo.item() - elbo)
    ratios = (e / (1e-6 * size), np.abs(g - grad).max() / (1e-4 * np.abs(grad).max()),
              np.abs(model.lam.cpu().numpy() - lam).max() / LAM_ATOL)
    print("%s: ELBO %.6g, error / tolerance: ELBO %.3g, grad %.3g, lam %.3g" % ((tag, elbo) + ratios))
    for name, r in zip(("update ELBO", "update grad", "update lam"), ratios):
        _note(name, r)
    assert e <= 1e-6 * size, (e, size)
    assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
    npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=LAM_ATOL)


def test_five_updates_track_the_reference_over_two_batches(ctx):
    from bayesic_amd.svi import StudentTReparamSVI
    S, B, D, seed, prec, a0, b0, nu = 11, 1029, 256, 1234, 2.0, 1.5, 0.5, 4.0
    batches = [_robust_data(B, D, 10 + k)[:4] for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, y0, o0, v0 = dev[0]
    model = StudentTReparamSVI(X0, y0, df=nu, n_total=10.0 * B, n_samples=S, seed=seed, lr=LR, prior_precision=prec,
                               a0=a0, b0=b0, ctx=ctx, offset=o0, weights=v0)
    lam = ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, STEPS + 1):
            k = (t - 1) % 2
            Xk, yk, ok, vk = dev[k]
            model.set_batch(Xk, yk, offset=ok, weights=vk)
            assert model.step() is None
            Xh, yh, oh, vh = batches[k]
            W_r, lp_r = ref.draw(lam, ref.noise(D, S, seed, t - 1))
            rho = lam[D + 1:].copy()
            lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, Xh, yh, nu, S, seed, 10.0 * B, LR, prec, a0, b0,
                                               offset=oh, weights=vh)
            size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(Xh, yh, W_r, lp_r, nu, oh, vh)[0], 10.0, prec, a0, b0, rho)
            _compare_step(ctx, model, lam, elbo, grad, size, "t=%d" % t)
    finally:
        ctx.call = real_call
    ctx.sync()
    assert calls.count(PASS) == STEPS and calls.count(FINISH) == STEPS
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_studentt_" not in c]
    p = model.params()
    var = math.exp(2.0 * lam[2 * D + 1])
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(lam[D] + 0.5 * var), rtol=1e-3)
    npt.assert_allclose(p["sigma_mean"], math.exp(-lam[D] + 0.5 * var), rtol=1e-3)
    assert p["df"] == nu


def test_five_full_covariance_updates_track_the_full_reference(ctx):
    """covariance="full" at D = 12: bsc_glm_scalar_fullrank_update on this pass's statistics next to the reference stepper
    of tests/_glm_scalar_full_ref.py with tests/_glm_studentt_ref.data_pass, the three tolerances of the mean-field test
    above."""
    from bayesic_amd.svi import StudentTReparamSVI
    B, D, S, seed, prec, a0, b0, scale, nu = 2000, 12, 8, 1234, 2.0, 1.5, 0.5, 10.0, 2.5
    P = D + 1
    X, y, o, v, _ = _robust_data(B, D, 10)
    model = StudentTReparamSVI(X, y, df=nu, n_total=scale * B, n_samples=S, seed=seed, lr=LR, prior_precision=prec,
                               a0=a0, b0=b0, ctx=ctx, offset=o, weights=v, covariance="full")
    lam = full_ref.init_lam(P)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for step in range(1, STEPS + 1):
            assert model.step() is None
            eps = ref.noise(D, S, seed, step - 1)
            W_r, lp_r = full_ref.draw(lam, eps)
            rho = lam[full_ref.diag_slots(P)]
            ell, G, T = ref.data_pass(X, y, W_r, lp_r, nu, o, v)
            lam, m1, m2, elbo, grad = full_ref.finish(lam, m1, m2, step, eps, W_r, lp_r, ell, G, T, scale, prec, a0, b0,
                                                      LR)
            size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(X, y, W_r, lp_r, nu, o, v)[0], scale, prec, a0, b0, rho)
            _compare_step(ctx, model, lam, elbo, grad, size, "full t=%d" % step)
    finally:
        ctx.call = real_call
    assert calls.count(PASS) == STEPS and calls.count("bsc_glm_scalar_fullrank_update") == STEPS
    assert FINISH not in calls
    p = model.params()
    L = p["L"]
    assert L.shape == (P, P) and (np.triu(L, 1) == 0).all() and np.abs(np.tril(L, -1)).max() > 0
    npt.assert_allclose(model.covariance(), L @ L.T, rtol=1e-14)
    var = float((L[D] ** 2).sum())                                     # the marginal variance of tau
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(p["m"][D] + 0.5 * var), rtol=1e-14)
    npt.assert_allclose(p["sigma_mean"], math.exp(-p["m"][D] + 0.5 * var), rtol=1e-12)


def test_raw_pointers_are_taken_as_they_are_and_tensors_are_checked(ctx):
    from bayesic_amd.svi import StudentTReparamSVI
    B, D = 325, 12
    X, y, o, v, _ = _robust_data(B, D, 7)
    Xd, yd, od, vd = (ctx.to_device(a) for a in (X, y, o, v))
    with pytest.raises(ValueError, match="y must be finite"):
        StudentTReparamSVI(Xd, yd / (yd - yd[0]), ctx=ctx)              # one 0 / 0
    a = StudentTReparamSVI(Xd, yd, df=2.5, ctx=ctx, offset=od, weights=vd)
    b = StudentTReparamSVI(Xd, yd, df=2.5, ctx=ctx)
    b.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())
    a.step()
    b.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        a.predict(Xd, yd)


# ---- 5. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, lis, nu, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, lis, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call(PREDICT, Xd, D, yd, od, B, D, Wd, pd, S, float(nu), *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, lis, nu, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, lis, nu, y, o, v)
    bnd = ref.predict_bounds(X, W, lis, nu, y, o, v)
    for k in keys:
        if k == "var" and nu <= 2.0:                        # no variance: +inf in every row, exactly
            assert np.isposinf(got[k]).all() and np.isposinf(want[k]).all()
            continue
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("studentt nu=%g %s: worst error / bound %.3g" % (nu, k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    X, y, W, lis, o, _ = ref.make_inputs(B, D, S, seed, mode="offset" if offset else "none")
    return X, y, W, lis, o


@pytest.mark.parametrize("B,D,S,shift,offset,nu", [(37, 12, 8, False, True, 4.0), (165, 12, 64, True, False, 1.0),
                                                   (37, 256, 8, True, True, 2.0), (1003, 256, 64, False, False, 2.5),
                                                   (325, 256, 8, False, False, 30.0), (165, 12, 64, False, True, 1.0e6),
                                                   (165, 200, 24, False, True, 4.0)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset, nu):
    X, y, W, lis, o = _predict_inputs(B, D, S, B + D + S, offset)
    assert lis.min() == ref.TAU_LO and lis.max() == ref.TAU_HI
    got = _predict(ctx, X, y, W, lis, nu, o, shift=shift)
    _assert_predict(got, X, y, W, lis, nu, o)
    if nu > 2.0:
        assert np.isfinite(got["var"]).all() and (got["var"] > 0).all()


def test_lpd_sum_is_in_its_fixed_order_and_predict_without_y_gives_the_moments_alone(ctx):
    X, y, W, lis, o = _predict_inputs(1003, 256, 24, 9)
    nu = 4.0
    full = _predict(ctx, X, y, W, lis, nu, o)
    again = _predict(ctx, X, y, W, lis, nu, o)
    for k in full:
        npt.assert_array_equal(full[k], again[k], err_msg=k)          # the same bits, the float64 sum included
    B, D = X.shape
    mean, var = (torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for _ in range(2))
    ctx.call(PREDICT, ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W), _dev_vec(ctx, lis), 24, nu,
             mean, var, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])
    npt.assert_array_equal(var.cpu().numpy(), full["var"])
    _assert_predict(dict(mean=mean.cpu().numpy(), var=var.cpu().numpy()), X, None, W, lis, nu, o, keys=("mean", "var"))
    got = _predict(ctx, X, y, W, lis, nu, o, want=("lpd_sum",))
    npt.assert_array_equal(got["lpd_sum"], full["lpd_sum"])
    assert (got["lpd"] == -777.0).all() and (got["mean"] == -777.0).all()
    # the sum of the float32 lpd vector in float64, whatever the order, to the roundings of that sum
    npt.assert_allclose(full["lpd_sum"][0], full["lpd"].astype(np.float64).sum(), rtol=1e-12)


def test_driver_predict_and_heldout_lpd(ctx):
    from bayesic_amd.svi import StudentTReparamSVI
    from bayesic_amd.svi import predict as mod
    B, D, nu = 600, 8, 4.0
    X, y, o, _, _ = _robust_data(B, D, 12)
    m = StudentTReparamSVI(X, y, df=nu, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "studentt"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the studentt model takes offset="):
        mod.predict(m, X, None, exposure=np.ones(B, np.float32))
    with pytest.raises(ValueError, match="belongs to the Weibull model, not studentt"):
        mod.predict(m, X, y, offset=o, upper=np.ones(B, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, offset=o, groups=np.zeros(B, np.int32))
    draws = mod.posterior_draws(m, 16)
    W, lis = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(lis, lp_r)
    out = m.predict(X, y, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, W, lis, nu, o)
    assert m.heldout_lpd(X, y, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    moments = m.predict(X, offset=o, draws=draws)
    assert set(moments) == {"mean", "var"}
    npt.assert_array_equal(moments["mean"].cpu().numpy(), got["mean"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, lis, nu, o, v)
    score = m.heldout_lpd(X, y, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    # the model's df goes to the pass: the same draws at another df give another density, that df's
    m.df = 1.0
    cauchy = {k: a.cpu().numpy() for k, a in m.predict(X, y, offset=o, draws=draws).items()}
    _assert_predict(cauchy, X, y, W, lis, 1.0, o)
    assert np.isposinf(cauchy["var"]).all() and np.abs(cauchy["lpd"] - got["lpd"]).max() > 0.1


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_come_from_the_shared_checks_with_their_codes_and_df_is_refused_by_name(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9) + 1.0, ctx.zeros((65, 260))
    o, v, lp = ctx.zeros(12), ctx.zeros(12), ctx.zeros(68)
    ell, G, T = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros(65, f64)
    out = ctx.zeros(9)

    def train(ldx, D, S, pa=lp, nu=4.0):
        ctx.call(PASS, X, ldx, y, o, v, 8, D, W, pa, S, nu, ell, G, T)

    def predict(ldx, D, S, pa=lp, nu=4.0):
        ctx.call(PREDICT, X, ldx, y, o, 8, D, W, pa, S, nu, out, None, None, None)

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
        for bad in (0.0, -4.0, float("nan"), float("inf"), 1e39, 1e-50):
            with pytest.raises(BayesicHipError, match="%s: df=" % who) as err:
                fn(256, 256, 8, nu=bad)
            assert "status -1:" in str(err.value)
    ctx.sync()
    assert float(ell.abs().sum().item()) == 0.0 and float(out.abs().sum().item()) == 0.0     # nothing was launched


# ---- 7. recovery ------------------------------------------------------------------------------------------------------------

def test_recovery_follows_the_reference_driver_and_the_outliers_hurt_the_gaussian_limit_more(ctx):
    """3000 rows, D = 8 with an intercept column, true sigma = 0.5, 10 % of the rows with their noise times 20; 300
    full-batch updates from one seed at nu = 4 and at nu = 1e6 (the Gaussian to six digits), on the device and in the
    float64 reference driver.  The fitted w and tau are held to the reference's within steps * lr * 1e-3 --
    tests/test_glm_lognormal_gpu.py's rule: an Adam step moves a coordinate by about lr at most, and the float32 pass's
    gradient error (held to 1e-4 of the largest entry above) is allowed to bend a thousandth of that path -- and
    sigma_mean = exp(-m_tau + e^{2 rho_tau} / 2) to what that allows.  Then the ORDERING alone: the error of the
    coefficients against the truth is smaller at nu = 4 than at nu = 1e6, in the reference and on the device (the
    contaminated rows carry noise of sd 10 into a least-squares fit; the t likelihood all but ignores them).  The
    figures are printed."""
    from bayesic_amd.svi import StudentTReparamSVI
    B, D, S, seed, steps, lr, prec, a0, b0 = 3000, 8, 8, 31, 300, 0.02, 1.0, 1.0, 0.1
    w_true = np.array([0.8, -0.6, 0.4, 0.3, -0.2, 0.5, -0.4, 0.1])
    X, y, o, _, bad = _robust_data(B, D, 5, sigma=0.5, outliers=0.1, blow=20.0, w=w_true, intercept=True)
    assert 0.08 < bad.mean() < 0.12
    tol = steps * lr * 1e-3
    fits = {}
    for nu in (4.0, 1.0e6):
        m = StudentTReparamSVI(X, y, df=nu, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0, b0=b0, ctx=ctx,
                               offset=o)
        for _ in range(steps):
            m.step()
        ctx.sync()
        lam_d = m.lam.cpu().numpy()
        lam_r = ref.fit(X, y, nu, S, seed, steps, lr, prec, a0, b0, offset=o)
        err = np.abs(lam_d[:D + 1] - lam_r[:D + 1]).max()
        var_r = math.exp(2.0 * lam_r[2 * D + 1])
        sigma_r = math.exp(-lam_r[D] + 0.5 * var_r)
        sigma_d = m.params()["sigma_mean"]
        sigma_tol = math.expm1(tol * (1.0 + var_r)) * (1.0 + 1e-6)
        print("nu=%g: sigma_mean dev %.5f ref %.5f, intercept dev %.5f ref %.5f, max |m dev - m ref| %.3g "
              "(tolerance %.3g), posterior sd %.3g .. %.3g" % (
                  nu, sigma_d, sigma_r, lam_d[0], lam_r[0], err, tol, np.exp(lam_r[D + 1:]).min(),
                  np.exp(lam_r[D + 1:]).max()))
        _note("recovery nu=%g" % nu, err / tol)
        assert err <= tol, (nu, err)
        assert abs(lam_d[0] - lam_r[0]) <= tol and abs(sigma_d / sigma_r - 1.0) <= sigma_tol
        fits[nu] = (np.abs(lam_d[:D] - w_true).max(), np.abs(lam_r[:D] - w_true).max(), sigma_d, sigma_r)
    (ed_t, er_t, sd_t, sr_t), (ed_g, er_g, sd_g, sr_g) = fits[4.0], fits[1.0e6]
    print("max |w - truth|: nu = 4 dev %.4f ref %.4f; nu = 1e6 dev %.4f ref %.4f; sigma_mean nu = 4 %.4f, nu = 1e6 %.4f"
          % (ed_t, er_t, ed_g, er_g, sd_t, sd_g))
    assert er_t < er_g and ed_t < ed_g


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
