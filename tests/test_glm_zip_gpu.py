"""GPU parity of the zero-inflated Poisson route (csrc/bsc_glm_zip.hip through the C ABI, svi/glm_zip.py, svi/predict.py)
against the float64 restatement in tests/_glm_zip_ref.py.

Tolerances:
 * ell, T and every entry of G: |dev - ref| <= EPS * bound quantity, EPS = 2e-5, the bound quantities per row v times the
   magnitudes of the terms added plus 1 (tests/_glm_zip_ref.py's docstring); rows of weight 0 are left out;
 * the limits l = +-80 on single rows: exact values at +80, the closed forms to float32 at -80;
 * the finish on supplied statistics: the bits of bsc_glm_nb_update on the same arguments and the reference at rtol 1e-9;
 * twenty updates against the reference driver: tests/test_glm_nb_gpu.py's three -- ELBO rtol 1e-6, gradient
   1e-4 * max|grad|, lam atol 2e-4;
 * the predictive: tests/_glm_zip_ref.predict_bounds.
A plain float32 replay of the link stays below 2.5e-7 of the bound quantities at these shapes and seeds, and EPS * bound
below 1e-3 of the results (tests/test_glm_zip_cpu.py); the measured ratios are printed.

Shapes: tests/_glm_zip_ref.PARITY_CASES, the smallest that reach each route, and two batches sized from the device's CU
count so that every wave runs two tiles.  tau uniform in [-8, 8], about half of the rows zero, every seventh positive
row a count in [100, 3000), a third of the zero rows pushed by the offset to mu in [1e-3, 50]; offset and weights each
null and each set, the rows of weight 0 holding NaN, infinity and negative values, ldx > D; sentinels of 1e30 behind y,
o, v and logodds."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch
from scipy.special import expit

import _glm_obs_ref as obs
import _glm_scalar_full_ref as full_ref
import _glm_zip_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30      # behind the end of y / o / v / logodds: a read past the end would wreck the sums
WORST = {}             # what: worst device error / (EPS * bound quantity) seen in this run (printed by each check)
PASS, FINISH, PREDICT = "bsc_glm_zip_data_pass", "bsc_glm_zip_update", "bsc_zip_predict_pass"


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, W, tau, o=None, v=None, ld=None, shift=()):
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
    pd = _dev_vec(ctx, tau, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64) + 5.0, ctx.zeros((S, D), torch.float64) + 5.0, ctx.zeros(S, torch.float64) + 5.0
    ctx.call(PASS, Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), float(ratio))


def _assert_close(got, X, y, W, tau, o, v, what=""):
    want = ref.data_pass(X, y, W, tau, o, v)
    bnd = ref.bounds(X, y, W, tau, o, v)
    ratios = []
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        assert np.isfinite(g).all(), name
        ratios.append(float((np.abs(g - w) / (ref.EPS * b + 1e-300)).max()))
        _note(name, ratios[-1])
    print("%s B=%d D=%d S=%d: error / tolerance ell %.3g, G %.3g, T %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], *ratios))
    for r, name in zip(ratios, ("ell", "G", "T")):
        assert r <= 1.0, (name, r)


def _check(ctx, X, y, W, tau, o, v, what="", **kw):
    assert ref.TAU_LO <= tau.min() and tau.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, W, tau, o, v, **kw)
    _assert_close(got, X, y, W, tau, o, v, what)
    return got


# ---- 1. parity at every route ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,mode,ld,shift,zeros", ref.PARITY_CASES)
def test_pass_matches_the_reference(ctx, B, D, S, mode, ld, shift, zeros):
    X, y, W, tau, o, v = ref.make_inputs(B, D, S, seed=ref.case_seed(B, D, S), mode=mode, zeros=zeros)
    if v is not None:
        dead = y[v == 0]
        assert np.isnan(dead).any() and np.isinf(dead).any() and (dead < 0).any()
    keep = np.ones(B, bool) if v is None else v > 0
    share = (y[keep] == 0).mean()
    assert share == zeros if zeros in (0.0, 1.0) else 0.4 < share < 0.65
    ell, G, T = _check(ctx, X, y, W, tau, o, v, what="zeros=%s" % zeros, ld=ld, shift=shift)
    if zeros == 1.0:
        assert (T > 0).all()                                    # every term a product of factors in [0, 1]
    if zeros == 0.0:
        wsum = float(B) if v is None else float(v.astype(np.float64).sum())
        npt.assert_allclose(T, -expit(tau.astype(np.float64)) * wsum, rtol=1e-5)     # -pi sum v


# ---- 2. every wave runs more than one tile ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("rows,D", [(16, 256), (8, 12)])
def test_two_tiles_per_wave_keep_tau_and_the_branch_with_their_rows(ctx, cu, rows, D):
    """B = one sweep of the resident waves (cu * 4 waves * 2 workgroups) + a few rows: T, the draw's tau, L1 and pi and the
    row's branch have to survive the hand-over from one tile to the next.  Every draw has its own tau, every row its own
    offset and weight; zero and positive rows alternate irregularly."""
    B = cu * 4 * rows * 2 + (5 if rows == 16 else 3)
    X, y, W, tau, o, v = ref.make_inputs(B, D, 8, seed=ref.case_seed(B, D, 8))
    assert len(set(tau.tolist())) == 8
    _check(ctx, X, y, W, tau, o, v, what="two tiles")


# ---- 3. the limits, the empty batch, the same bits run to run ---------------------------------------------------------------

TAUS = np.array([-8.0, -3.0, -0.5, 0.0, 0.5, 2.0, 5.0, 8.0], np.float32)


def _single_row(ctx, l, yv, D):
    """One row whose logit is exactly l at every draw: W = 0 and the offset carries it."""
    X = np.linspace(-1.0, 1.0, D, dtype=np.float32)[None, :]
    W = np.zeros((8, D), np.float32)
    return X, _pass(ctx, X, np.array([yv], np.float32), W, TAUS, np.array([l], np.float32), None)


@pytest.mark.parametrize("D", [12, 256])
def test_a_zero_row_at_l_plus_80_gives_exactly_log_pi_zero_and_one_minus_pi(ctx, D):
    f = np.float32
    t64 = TAUS.astype(np.float64)
    L1 = (np.maximum(t64, 0.0) + np.log1p(np.exp(-np.abs(t64)))).astype(f)      # float64 once per launch, then rounded
    pi = expit(t64).astype(f)
    _, (ell, G, T) = _single_row(ctx, 80.0, 0.0, D)
    npt.assert_array_equal(ell, (TAUS - L1).astype(np.float64))
    npt.assert_allclose(ell, np.log(expit(t64)), atol=1e-6)                     # ... which is log pi
    assert (G == 0).all()
    npt.assert_array_equal(T, (f(1.0) - pi).astype(np.float64))


@pytest.mark.parametrize("D,yv", [(12, 0.0), (12, 3.0), (256, 0.0), (256, 3.0)])
def test_rows_at_l_minus_80_are_finite_and_equal_the_closed_forms(ctx, D, yv):
    X, (ell, G, T) = _single_row(ctx, -80.0, yv, D)
    lp, dl, dt = ref.link(np.full(8, -80.0), np.full(8, yv), TAUS.astype(np.float64))
    assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(T).all()
    npt.assert_allclose(ell, lp, rtol=2e-6, atol=2e-6)           # (a zero row: -(1 - pi) mu, 0 to a rounding of L1)
    npt.assert_allclose(G, dl[:, None] * X.astype(np.float64), rtol=1e-6, atol=1e-37)
    npt.assert_allclose(T, dt, rtol=1e-6, atol=1e-7)
    if yv == 0.0:
        assert (T >= 0).all()


def test_an_empty_batch_gives_zeros(ctx):
    S, D = 11, 64
    W, tau = ctx.zeros((S, D)), ctx.zeros(S)
    ell, G, T = (torch.full(s, 7.0, dtype=torch.float64, device=ctx.device) for s in ((S,), (S, D), (S,)))
    ctx.call(PASS, None, D, None, None, None, 0, D, W, tau, S, ell, G, T)
    ctx.sync()
    assert not ell.any() and not G.any() and not T.any()


def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (517, 200, 8, 6)):
        X, y, W, tau, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, tau, o, v)
        b = _pass(ctx, X, y, W, tau, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


# ---- 4. the finish ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S", [(256, 8), (12, 11)])
def test_the_mean_field_finish_on_supplied_statistics(ctx, D, S):
    """bsc_glm_zip_update and bsc_glm_nb_update run one body: the same arguments give the same bits, and they are the
    reference's update."""
    f64 = torch.float64
    P = D + 1
    rs = np.random.RandomState(D + S)
    seed, t = 77, 4
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, lo = ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(2 * P), 0.01 * rs.uniform(size=2 * P)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, _, _, elbo_r, grad_r = ref.update(lam, m1.copy(), m2.copy(), t, eps, W, lo, ell, G, T, scale, prec, a0, b0,
                                             lr)

    def run(name):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W=ctx.to_device(W.ravel()), lp=_dev_vec(ctx, lo),
                 W_n=ctx.zeros(S * D), lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64),
                 stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
        ctx.call(name, d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["lp"], D, S, scale, prec,
                 a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"], d["elbo"], d["grad"])
        ctx.sync()
        return {k: a.cpu().numpy() for k, a in d.items()}

    h, twin = run(FINISH), run("bsc_glm_nb_update")
    for k in ("elbo", "grad", "out", "m1", "m2", "W_n", "lp_n"):
        npt.assert_array_equal(h[k], twin[k], err_msg=k)
    npt.assert_allclose(h["elbo"][0], elbo_r, rtol=1e-9)
    npt.assert_allclose(h["out"], lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(h["grad"], grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())


def test_the_full_covariance_finish_on_supplied_statistics_and_in_the_driver(ctx):
    """The full guide needs no kernel of this family's: bsc_glm_scalar_fullrank_update on supplied statistics against
    tests/_glm_scalar_full_ref.finish (rtol 1e-9), then covariance="full" at D = 12, ten updates next to that reference
    stepper with tests/_glm_zip_ref.data_pass, the three tolerances of the mean-field test below."""
    from bayesic_amd.svi import ZIPoissonReparamSVI
    f64 = torch.float64
    D, S, seed, t = 12, 8, 77, 4
    P = D + 1
    rs = np.random.RandomState(3)
    Lf = np.tril(0.05 * rs.standard_normal((P, P)), -1) + np.diag(np.exp(-2.0 + 0.3 * rs.standard_normal(P)))
    lam = full_ref.pack(0.1 * rs.standard_normal(P), Lf)
    n = lam.size
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, lo = full_ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(n), 0.01 * rs.uniform(size=n)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, _, _, elbo_r, grad_r = full_ref.finish(lam, m1.copy(), m2.copy(), t, eps, W, lo, ell, G, T, scale, prec, a0,
                                                  b0, lr)
    d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(n, f64), m1=ctx.to_device(m1, f64), m2=ctx.to_device(m2, f64),
             eps=ctx.to_device(eps.ravel(), f64), eps_n=ctx.to_device(eps_n.ravel(), f64),
             W=ctx.to_device(np.ascontiguousarray(W).ravel()), lp=_dev_vec(ctx, lo), W_n=ctx.zeros(S * D),
             lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(n, f64),
             stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
    ctx.call("bsc_glm_scalar_fullrank_update", d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"],
             d["lp"], D, S, scale, prec, a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"],
             d["elbo"], d["grad"])
    ctx.sync()
    npt.assert_allclose(d["elbo"].cpu().numpy()[0], elbo_r, rtol=1e-9)
    npt.assert_allclose(d["out"].cpu().numpy(), lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(d["grad"].cpu().numpy(), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())

    B, seed, lr, prec, a0, b0, scale = 2000, 1234, 0.01, 2.0, 1.5, 0.5, 10.0
    X, y, o, v = _count_data(B, D, 10, shift=-1.5)           # (the ELBO of the size of its terms: the test below says why)
    model = ZIPoissonReparamSVI(X, y, n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0,
                                b0=b0, ctx=ctx, offset=o, weights=v, covariance="full")
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
            ell, G, T = ref.data_pass(X, y, W_r, lp_r, o, v)
            lam, m1, m2, elbo, grad = full_ref.finish(lam, m1, m2, step, eps, W_r, lp_r, ell, G, T, scale, prec, a0, b0,
                                                      lr)
            size = scale * ref.bounds(X, y, W_r, lp_r, o, v)[0].mean()
            assert size <= 4.0 * abs(elbo), size / abs(elbo)
            ctx.sync()
            g = model.grad.cpu().numpy()
            print("full t=%d: ELBO %.6g, rel error %.3g; grad err/max %.3g, lam err %.3g" % (
                step, elbo, abs(model.elbo.item() - elbo) / abs(elbo), np.abs(g - grad).max() / np.abs(grad).max(),
                np.abs(model.lam.cpu().numpy() - lam).max()))
            npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
            assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert calls.count(PASS) == 10 and calls.count("bsc_glm_scalar_fullrank_update") == 10 and FINISH not in calls
    p = model.params()
    L = p["L"]
    assert L.shape == (P, P) and (np.triu(L, 1) == 0).all() and np.abs(np.tril(L, -1)).max() > 0
    var = float((L[D] ** 2).sum())                                     # the marginal variance of tau
    npt.assert_allclose(p["odds_mean"], math.exp(p["m"][D] + 0.5 * var), rtol=1e-14)
    npt.assert_allclose(p["zero_share_mean"], ref.zero_share_mean(p["m"][D], var), rtol=1e-9)


# ---- 5. the driver ----------------------------------------------------------------------------------------------------------

def _count_data(B, D, seed, pi=0.3, shift=0.5):
    """tests/test_glm_nb_gpu.py's regression data with zero-inflated Poisson counts: offsets N(shift, 0.5^2), so that
    the Poisson part has a mean near e^shift, a structural-zero share pi, weights U(0, 2) with every sixth exactly 0."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.5 * rs.standard_normal(B) + shift).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    mu = np.exp(X.astype(np.float64) @ rs.standard_normal(D) + o)
    y = rs.poisson(mu).astype(np.float32)
    y[rs.uniform(size=B) < pi] = 0.0
    return X, y, o, v


@pytest.mark.parametrize("S", [8, 11])
def test_twenty_updates_track_the_reference_over_two_batches(ctx, S):
    """tests/test_glm_nb_gpu.py's test, its data recipe and its three tolerances.  The ELBO leaves -lnGamma(y + 1) out,
    so with counts of mean 1.6 its positive y l terms and its negative ones nearly cancel (on the reference stepper the
    ELBO changes sign between the batches, 50 to 90 times smaller than the sum of its terms' sizes).  With the offsets
    of that test (shift -1.5: counts of mean 0.25, 81 % zeros) the ELBO is of the size of its terms and its rtol is a
    statement about the pass: the condition number scale * sum of the bound quantities / |ELBO|, from reference
    quantities alone, is asserted to stay below 4 as there (it is 3.4 .. 3.8)."""
    from bayesic_amd.svi import ZIPoissonReparamSVI
    B, D, seed, lr, prec, a0, b0 = 1029, 256, 1234, 0.01, 2.0, 1.5, 0.5
    batches = [_count_data(B, D, 10 + k, shift=-1.5) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, y0, o0, v0 = dev[0]
    model = ZIPoissonReparamSVI(X0, y0, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0,
                                b0=b0, ctx=ctx, offset=o0, weights=v0)
    lam = ref.init_lam(D)
    assert lam[D] == 0.0                                       # tau starts at 0: pi = 1/2
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
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
            W_r, lp_r = ref.draw(lam, ref.noise(D, S, seed, t - 1))
            lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, Xh, yh, S, seed, 10.0 * B, lr, prec, a0, b0, offset=oh,
                                               weights=vh)
            if t in (1, 2, 3, 10, 20):
                size = 10.0 * ref.bounds(Xh, yh, W_r, lp_r, oh, vh)[0].mean()
                ctx.sync()
                g = model.grad.cpu().numpy()
                print("t=%d: ELBO %.6g, condition %.2f, rel error %.3g; grad err/max %.3g; lam err %.3g" % (
                    t, elbo, size / abs(elbo), abs(model.elbo.item() - elbo) / abs(elbo),
                    np.abs(g - grad).max() / np.abs(grad).max(), np.abs(model.lam.cpu().numpy() - lam).max()))
                assert size <= 4.0 * abs(elbo), size / abs(elbo)
                npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    ctx.sync()
    assert PASS in calls and FINISH in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_zip_" not in c]
    p = model.params()
    var = math.exp(2.0 * lam[2 * D + 1])
    npt.assert_allclose(p["odds_mean"], math.exp(lam[D] + 0.5 * var), rtol=1e-3)
    npt.assert_allclose(p["zero_share_mean"], ref.zero_share_mean(lam[D], var), rtol=1e-3)


def test_driver_checks_the_batch_outside_step_and_takes_exposure_and_weights(ctx):
    from bayesic_amd.svi import ZIPoissonReparamSVI
    B, D = 325, 12
    X, y, o, v = _count_data(B, D, 7)
    Xd, yd, od, vd = (ctx.to_device(a) for a in (X, y, o, v))
    with pytest.raises(ValueError, match="y must be finite, >= 0 and whole"):
        ZIPoissonReparamSVI(Xd, yd + 0.5, ctx=ctx)
    with pytest.raises(ValueError, match="y must be finite, >= 0 and whole"):
        ZIPoissonReparamSVI(Xd, yd - 1.0, ctx=ctx)
    a = ZIPoissonReparamSVI(Xd, yd, ctx=ctx, offset=od, weights=vd)
    b = ZIPoissonReparamSVI(Xd, yd, ctx=ctx, exposure=torch.exp(od), weights=vd)
    npt.assert_allclose(b.offset.cpu().numpy(), o, rtol=1e-5, atol=1e-6)           # kept as log(exposure)
    c = ZIPoissonReparamSVI(Xd, yd, ctx=ctx)
    with pytest.raises(ValueError, match="y must be finite, >= 0 and whole"):
        c.set_batch(Xd, yd + 0.25)
    c.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())
    a.step()
    c.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), c.lam.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        a.predict(Xd, yd)


# ---- 6. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, tau, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, tau, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call(PREDICT, Xd, D, yd, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, tau, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, tau, y, o, v)
    bnd = ref.predict_bounds(X, W, tau, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        _note("predict " + k, worst)
        print("zip %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    """make_inputs with the logits kept at |l| <= 3.5 (the predictive mean holds exp(l))."""
    X, y, W, tau, o, _ = ref.make_inputs(B, D, S, seed, mode="offset")
    peak = np.abs(obs.logits(X, W, o)).max()
    if peak > 3.5:
        W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    assert (y > 0).any() and (y == 0).any()
    return X, y, W, tau, (o if offset else None)


@pytest.mark.parametrize("B,D,S,shift,offset", [(37, 12, 8, False, True), (165, 12, 64, True, False),
                                                (37, 256, 8, True, True), (1003, 256, 64, False, False),
                                                (325, 256, 8, False, False), (165, 12, 64, False, True)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset):
    X, y, W, tau, o = _predict_inputs(B, D, S, B + D + S, offset)
    got = _predict(ctx, X, y, W, tau, o, shift=shift)
    _assert_predict(got, X, y, W, tau, o)


def test_predict_without_y_gives_the_moments_alone_and_the_optional_outputs(ctx):
    X, y, W, tau, o = _predict_inputs(165, 12, 8, 9)
    full = _predict(ctx, X, y, W, tau, o)
    B, D = X.shape
    mean, var = (torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for _ in range(2))
    ctx.call(PREDICT, ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W), _dev_vec(ctx, tau), 8, mean,
             var, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])
    npt.assert_array_equal(var.cpu().numpy(), full["var"])
    _assert_predict(dict(mean=mean.cpu().numpy(), var=var.cpu().numpy()), X, None, W, tau, o, keys=("mean", "var"))
    got = _predict(ctx, X, y, W, tau, o, want=("lpd_sum",))
    npt.assert_array_equal(got["lpd_sum"], full["lpd_sum"])
    assert (got["lpd"] == -777.0).all() and (got["mean"] == -777.0).all()
    got = _predict(ctx, X, y, W, tau, o, want=("lpd",))
    npt.assert_array_equal(got["lpd"], full["lpd"])
    assert (got["lpd_sum"] == -777.0).all() and (got["var"] == -777.0).all()


def test_the_lpd_is_finite_at_l_plus_and_minus_80(ctx):
    """W = 0, the offset carries the logit: lpd of a zero and of a positive count at l = +-80 against the closed forms
    (at +80 a zero row's is the log of the draw average of pi, a count of 3 has log p near -e^80 and stays finite)."""
    D = 12
    X = np.linspace(-1.0, 1.0, 4 * D, dtype=np.float32).reshape(4, D)
    W = np.zeros((8, D), np.float32)
    o = np.array([80.0, 80.0, -80.0, -80.0], np.float32)
    y = np.array([0.0, 3.0, 0.0, 3.0], np.float32)
    got = _predict(ctx, X, y, W, TAUS, o, want=("lpd",))["lpd"]
    want = ref.predict(X, W, TAUS, y, o)["lpd"]
    assert np.isfinite(got).all()
    npt.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    npt.assert_allclose(got[0], math.log(expit(TAUS.astype(np.float64)).mean()), rtol=1e-6)


def test_driver_predict_heldout_lpd_and_zero_probability(ctx):
    from bayesic_amd.svi import ZIPoissonReparamSVI
    from bayesic_amd.svi import predict as mod
    B, D = 600, 8
    X, y, o, _ = _count_data(B, D, 12)
    m = ZIPoissonReparamSVI(X, y, exposure=np.exp(o), n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "zip"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    with pytest.raises(ValueError, match="belongs to the Weibull model, not zip"):
        mod.predict(m, X, y, offset=o, upper=np.ones(B, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, offset=o, groups=np.zeros(B, np.int32))
    draws = mod.posterior_draws(m, 16)
    W, tau = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(tau, lp_r)
    assert tau.shape == (16,)
    out = m.predict(X, y, offset=o, draws=draws)
    got = {k: a.cpu().numpy() for k, a in out.items()}
    _assert_predict(got, X, y, W, tau, o)
    assert m.heldout_lpd(X, y, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    # exposure = e^offset gives the offset's results to the rounding of its logarithm
    oute = m.predict(X, y, exposure=np.exp(o), draws=draws)
    oe = np.log(np.exp(o)).astype(np.float32)
    _assert_predict({k: a.cpu().numpy() for k, a in oute.items()}, X, y, W, tau, oe)
    moments = m.predict(X, offset=o, draws=draws)
    assert set(moments) == {"mean", "var"}
    npt.assert_array_equal(moments["mean"].cpu().numpy(), got["mean"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, tau, o, v)
    score = m.heldout_lpd(X, y, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    # zero_probability: exp of the lpd at y = 0, within that lpd's bound (d e^x = e^x dx, and one rounding)
    p0 = m.zero_probability(X, offset=o, draws=draws)
    assert p0.dtype == torch.float32 and tuple(p0.shape) == (B,)
    p0 = p0.cpu().numpy()
    p_ref = ref.zero_probability(X, W, tau, o)
    tol = p_ref * ref.predict_bounds(X, W, tau, np.zeros(B, np.float32), o)["lpd"] + ref.EPS * p_ref
    _note("zero_probability", np.max(np.abs(p0 - p_ref) / tol))
    assert (np.abs(p0 - p_ref) <= tol).all(), np.max(np.abs(p0 - p_ref) / tol)
    assert (p0 > expit(tau.astype(np.float64)).mean() - 1e-6).all() and (p0 <= 1.0).all()    # never below the zero share
    # a model fitted without an offset predicts without one
    m0 = ZIPoissonReparamSVI(X, y, n_samples=8, seed=9, ctx=ctx)
    m0.step()
    d0 = mod.posterior_draws(m0, 40)
    g0 = {k: a.cpu().numpy() for k, a in m0.predict(X, y, draws=d0).items()}
    _assert_predict(g0, X, y, d0[0].cpu().numpy(), d0[1].cpu().numpy(), None)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point(ctx):
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
        with pytest.raises(BayesicHipError, match="%s: logodds is null" % who) as err:
            fn(256, 256, 8, pa=None)
        assert "status -1:" in str(err.value)
    with pytest.raises(BayesicHipError, match="%s: stats is null" % FINISH):
        ctx.call(FINISH, None, ell, ell, ell, ell, ell, W, lp, 12, 8, 1.0, 1.0, 1.0, 1.0, 1, 0.01, 0.9, 0.999, 1e-8, 1, 1,
                 ell, 1, W, lp, ell, ell)
    ctx.sync()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------


def test_end_to_end_recovery_follows_the_reference_driver_and_beats_the_poisson_fit_held_out(ctx):
    """3 000 simulated rows, D = 8 with an intercept column, pi = 0.3, mu near 2; 300 full-batch updates from one seed.
    The reference driver (float64, on the CPU) ends at an intercept of 0.64321 with a posterior standard deviation of
    0.02644, tau = -0.94117 (sd 0.05638) and zero_share_mean = 0.28080, whose standard deviation is by the delta method
    pi (1 - pi) sd_tau = 0.2808 * 0.7192 * 0.05638 = 0.01139.  The device's zero_share_mean and intercept must lie within
    three of those standard deviations of the reference's values: the reference, not the truth (0.3 and 0.693), sets the
    mark.  On the 1 000 held-out rows heldout_lpd of this fit must exceed that of GLMReparamSVI(link="poisson") fitted
    to the same rows the same way; the margin is printed.  Measured on an MI355X: the device ends at the reference's
    figures to five digits (intercept 0.64321, tau -0.94117, zero_share_mean 0.28080); held-out lpd per row -1.5641
    (ZIP) against -1.6798 (Poisson, whose intercept has gone down to 0.316), a margin of 0.1157 nats per row."""
    from bayesic_amd.svi import GLMReparamSVI, ZIPoissonReparamSVI
    c, r = ref.E2E, ref.E2E_REF
    REF_INTERCEPT, REF_INTERCEPT_SD, REF_TAU, REF_TAU_SD = r["intercept"], r["intercept_sd"], r["tau"], r["tau_sd"]
    REF_ZERO_SHARE = r["zero_share"]
    X, y = ref.simulate(c["B"], c["D"], c["seed"])
    n = c["fit_rows"]
    Xf, yf, Xh, yh = X[:n], y[:n], X[n:], y[n:]
    kw = dict(n_samples=c["S"], seed=c["vi_seed"], lr=c["lr"], prior_precision=c["prec"], ctx=ctx)
    m = ZIPoissonReparamSVI(Xf, yf, a0=c["a0"], b0=c["b0"], **kw)
    pois = GLMReparamSVI(Xf, yf, link="poisson", **kw)
    for _ in range(c["steps"]):
        m.step()
        pois.step()
    ctx.sync()
    p = m.params()
    share_sd = REF_ZERO_SHARE * (1.0 - REF_ZERO_SHARE) * REF_TAU_SD
    print("intercept %.5f (reference %.5f, sd %.5f); tau %.5f (reference %.5f); zero_share_mean %.5f (reference %.5f, sd "
          "%.5f)" % (p["m"][0], REF_INTERCEPT, REF_INTERCEPT_SD, p["m"][c["D"]], REF_TAU, p["zero_share_mean"],
                     REF_ZERO_SHARE, share_sd))
    _note("recovery intercept", abs(p["m"][0] - REF_INTERCEPT) / (3.0 * REF_INTERCEPT_SD))
    _note("recovery zero share", abs(p["zero_share_mean"] - REF_ZERO_SHARE) / (3.0 * share_sd))
    assert abs(p["m"][0] - REF_INTERCEPT) <= 3.0 * REF_INTERCEPT_SD
    assert abs(p["zero_share_mean"] - REF_ZERO_SHARE) <= 3.0 * share_sd
    zip_lpd, pois_lpd = m.heldout_lpd(Xh, yh, seed=1), pois.heldout_lpd(Xh, yh, seed=1)
    print("held-out lpd per row: ZIP %.4f, Poisson %.4f, margin %.4f; Poisson intercept %.4f" % (
        zip_lpd, pois_lpd, zip_lpd - pois_lpd, pois.lam.cpu().numpy()[0]))
    assert zip_lpd > pois_lpd


@pytest.fixture(scope="module", autouse=True)
def _report_the_worst_ratios():
    """After the module: what its checks measured in this run (visible with -s)."""
    yield
    for k in sorted(WORST):
        print("worst %s: %.3g of its tolerance" % (k, WORST[k]))
