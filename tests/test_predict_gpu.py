"""GPU parity of the posterior predictive (csrc/bsc_predict.hip through the C ABI, svi/predict.py, the drivers and the
plugin route) against the float64 restatement in tests/_predict_ref.py.

Bounds use float64 reference quantities and the project's factor 2e-5 only (test_glm_gpu / test_bbvi_gpu's bound for
a float32 dot of <= 256 terms plus one transcendental).  With a_ns = sum_d |x_nd w_sd| and r = y - l:
 * per-draw error of log p:  e_ns = 2e-5 (|y l| + A(l) + 1) for the GLM links,
                             e_ns = 2e-5 (e^{-logvar} (|r| (a_ns + |y|) + r^2) + |logvar| + 1) for the Gaussian;
 * |lpd_n - ref| <= max_s e_ns (log-mean-exp is 1-Lipschitz in the max norm), |lpd_sum - ref| <= sum_n max_s e_ns;
 * per-draw error of mu: m_ns = 2e-5 (mu'(l_ns) a_ns + |mu(l_ns)|), so |mean_n - ref| <= mean_s m_ns;
 * var_n = mean_s v_ns + mean_s (mu_ns - mean_n)^2.  The first term moves by at most mean_s u_ns with u_ns the
   per-draw error of v: 2e-5 v (Gaussian: one exponential), 2e-5 (|1 - 2 mu| mu' a + v) (logistic: v = mu (1 - mu)
   through the chain rule), m_ns (Poisson: v = mu).  The second by mean_s 2 |mu_ns - mean_n| (m_ns + mean_s' m_ns')
   (each factor of the square moves by the error of mu_ns plus that of the mean) plus 2e-5 of itself for the
   float32 squares and sum.  The bound is the sum of the three.
Poisson inputs keep |l| <= 4 (asserted on the float64 logits); the Gaussian family uses logvar in [-2, 1].

End to end (float64 reference of the same runs, tests/_glm_ref.py / oracle.svi / tests/_fullrank_ref.py, S = 64
predictive draws, 1000 held-out rows; recorded before the device ran):
 * logistic, D = 8, AR(0.9) design, 300 updates at lr 0.05, S = 8: heldout_lpd -0.7022 at t = 0, -0.4680 fitted,
   constant-rate baseline -0.6923;
 * linear-Gaussian (oracle.svi.make_cfg2's model, AR(0.9) design), 450 updates at lr 0.02, S = 32: -1.4212 at t = 0,
   mean-field -0.7691, full -0.7678, constant Gaussian baseline -1.4204; full - mean-field = +0.0013 per row with
   a standard error of 0.0004 from the per-row differences."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _fullrank_ref as fr
import _glm_ref as glm_ref
import _predict_ref as ref

pytestmark = pytest.mark.gpu

FAMILIES = ref.FAMILIES
SENTINEL = -777.0


def _run(ctx, family, X, y, W, logvar, ld=None, want=("mean", "var", "lpd", "lpd_sum"), y_offset=False):
    """bsc_predict_pass on host arrays; outputs not in ``want`` are passed as NULL.  Returns dict of numpy arrays."""
    B, D = X.shape
    S = W.shape[0]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    yd = None
    if y is not None:
        yd = ctx.to_device(np.concatenate([[9.0], y]).astype(np.float32))[1:] if y_offset else ctx.to_device(y)
    Wd = ctx.to_device(W)
    lvd = None if logvar is None else ctx.to_device(logvar)
    out = {k: torch.full((B,), SENTINEL, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), SENTINEL, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call("bsc_predict_pass", ref.CODE[family], Xd, (ld or D), yd, B, D, Wd, lvd, S, *args)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _inputs(family, B, D, S, seed):
    """test_glm_gpu._inputs' recipe, restated, with a Gaussian case added."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    logvar = None
    if family == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    elif family == "poisson":
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(X.astype(np.float64) @ W.astype(np.float64).T).max() if B else 0.0
        if peak > 3.5:
            W = (W * (3.5 / peak)).astype(np.float32)
    else:
        y = rs.standard_normal(B).astype(np.float32)
        logvar = rs.uniform(-2.0, 1.0, S).astype(np.float32)
    return X, y, W, logvar


def _check(ctx, family, X, y, W, logvar, **kw):
    got = _run(ctx, family, X, y, W, logvar, **kw)
    B = X.shape[0]
    if B == 0:
        assert got["lpd_sum"][0] == 0.0
        return got
    want = ref.predict(family, X, W, logvar, y)
    bnd = ref.bounds(family, X, W, logvar, y)
    if family == "poisson":
        assert np.abs(ref.logits(X, W)).max() <= 4.0
    worst = {}
    for k in ("mean", "var", "lpd", "lpd_sum"):
        err = np.abs(got[k] - want[k])
        worst[k] = float(np.max(err / (bnd[k] + 1e-300)))
    print("%s B=%d D=%d S=%d: worst error / bound  mean %.3g  var %.3g  lpd %.3g  lpd_sum %.3g" % (
        family, B, X.shape[1], W.shape[0], worst["mean"], worst["var"], worst["lpd"], worst["lpd_sum"]))
    for k, w in worst.items():
        assert w <= 1.0, (k, w)
    return got


@pytest.mark.parametrize("S", [1, 3, 8, 9, 16, 64])
@pytest.mark.parametrize("B,D", [(0, 256), (5, 256), (32, 256), (1003, 256), (4099, 64), (777, 4), (20000, 252)])
@pytest.mark.parametrize("family", FAMILIES)
def test_pass_matches_the_reference(ctx, family, B, D, S):
    X, y, W, logvar = _inputs(family, B, D, S, seed=B * 7 + D + S)
    _check(ctx, family, X, y, W, logvar)


@pytest.mark.parametrize("B,D,ld", [(333, 64, 96), (1003, 256, 260), (50, 256, 512)])
@pytest.mark.parametrize("family", FAMILIES)
def test_pass_respects_the_leading_dimension(ctx, family, B, D, ld):
    X, y, W, logvar = _inputs(family, B, D, 8, seed=ld)
    _check(ctx, family, X, y, W, logvar, ld=ld)


@pytest.mark.parametrize("family", FAMILIES)
def test_y_that_is_not_16_byte_aligned(ctx, family):
    X, y, W, logvar = _inputs(family, 1003, 256, 8, seed=3)
    _check(ctx, family, X, y, W, logvar, y_offset=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_each_output_is_optional_and_the_others_do_not_change(ctx, family):
    X, y, W, logvar = _inputs(family, 1003, 256, 16, seed=8)
    full = _run(ctx, family, X, y, W, logvar)
    names = ("mean", "var", "lpd", "lpd_sum")
    for drop in names:
        got = _run(ctx, family, X, y, W, logvar, want=tuple(k for k in names if k != drop))
        assert (got[drop] == SENTINEL).all()
        for k in names:
            if k != drop:
                npt.assert_array_equal(got[k], full[k])
    nol = _run(ctx, family, X, None, W, logvar, want=("mean", "var"))     # no y at all
    npt.assert_array_equal(nol["mean"], full["mean"])
    npt.assert_array_equal(nol["var"], full["var"])


@pytest.mark.parametrize("D,S", [(256, 8), (256, 64), (64, 24)])
def test_operand_layout_with_exact_integers(ctx, D, S):
    """One-hot rows (row n has its 1 in column 3 n mod D) and draws that look at the columns d = s mod 8 with weight
    s + 1: l[n, s] is s + 1 or 0 and WHICH draws see a row changes with the row, so any mix-up of row, draw or column
    changes the result.  Gaussian family: mean_n = sum of small integers / S is exact in float32; lpd at rtol 1e-6."""
    B = 96
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), (3 * np.arange(B)) % D] = 1.0
    W = np.zeros((S, D), np.float32)
    for s in range(S):
        W[s, s % 8::8] = s + 1.0
    y = (np.arange(B) % 5).astype(np.float32)
    logvar = np.zeros(S, np.float32)
    got = _run(ctx, "gaussian", X, y, W, logvar)
    want = ref.predict("gaussian", X, W, logvar, y)
    npt.assert_array_equal(got["mean"], want["mean"].astype(np.float32))
    npt.assert_allclose(got["var"], want["var"], rtol=1e-6)
    npt.assert_allclose(got["lpd"], want["lpd"], rtol=1e-6)
    L = ref.logits(X, W)
    assert len(set(np.round(want["mean"], 6))) >= 8 and len({tuple(r) for r in L}) >= 8 and len({tuple(c) for c in L.T}) == S


@pytest.mark.parametrize("S", [8, 64])
def test_variance_is_centred(ctx, S):
    """l_ns = 1000 + (s mod 8), logvar = 0: var = 1 + 5.25.  E[mu^2] - E[mu]^2 in float32 misses this by about 2 %."""
    D, B = 256, 40
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), (7 * np.arange(B)) % D] = 1.0
    W = np.tile((1000.0 + (np.arange(S) % 8))[:, None], (1, D)).astype(np.float32)
    got = _run(ctx, "gaussian", X, None, W, np.zeros(S, np.float32), want=("mean", "var"))
    npt.assert_allclose(got["var"], 6.25, rtol=1e-5)
    npt.assert_allclose(got["mean"], 1003.5, rtol=1e-6)


def test_logistic_at_extreme_logits(ctx):
    D, B, S = 256, 200, 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    sign = (-1.0) ** (np.arange(D)[None, :] + np.zeros((S, 1)))
    W = (80.0 * sign).astype(np.float32)
    y = ((np.arange(B) // 2) % 2).astype(np.float32)
    got = _run(ctx, "logistic", X, y, W, None)
    L = ref.logits(X, W)
    assert set(np.unique(L)) == {-80.0, 80.0} and len({(a, b) for a, b in zip(L[:, 0], y)}) == 4
    want = ref.predict("logistic", X, W, None, y)
    assert np.isfinite(got["lpd"]).all() and np.isfinite(got["mean"]).all() and np.isfinite(got["var"]).all()
    assert np.abs(got["lpd"] - want["lpd"]).max() <= 2e-5 * 81


def test_lpd_is_log_mean_exp_not_mean_log(ctx):
    """One draw with log p ~ -0.1, seven with log p ~ -60 (y = 1, l = 2.3 or -60)."""
    D, B, S = 64, 33, 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    W = np.full((S, D), -60.0, np.float32)
    W[5, :] = 2.3
    y = np.ones(B, np.float32)
    got = _run(ctx, "logistic", X, y, W, None)
    L = ref.logits(X, W)
    want = ref.predict("logistic", X, W, None, y)
    npt.assert_allclose(want["lpd"], -math.log1p(math.exp(-2.3)) - math.log(8), rtol=1e-6)
    npt.assert_allclose(got["lpd"], want["lpd"], rtol=1e-5)
    assert (got["lpd"] - ref.log_p("logistic", L, y).mean(axis=1) > 40).all()


def test_two_calls_are_bit_identical(ctx):
    X, y, W, logvar = _inputs("poisson", 20000, 252, 16, seed=1)
    a, b = _run(ctx, "poisson", X, y, W, None), _run(ctx, "poisson", X, y, W, None)
    for k in a:
        npt.assert_array_equal(a[k], b[k])


def test_refusals_name_the_quantity_and_leave_the_outputs_alone(ctx):
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    Xb = torch.zeros((9, 264), dtype=torch.float32, device=dev)
    Wb = torch.zeros((65 * 264 + 4,), dtype=torch.float32, device=dev)
    y, lv = torch.zeros(9, dtype=torch.float32, device=dev), torch.zeros(65, dtype=torch.float32, device=dev)
    out = [torch.full((9,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    out.append(torch.full((1,), SENTINEL, dtype=torch.float64, device=dev))

    def call(match, status, family=0, X=Xb, ldx=264, yy=y, D=256, W=Wb, logvar=lv, S=8, outs=None):
        with pytest.raises(BayesicHipError, match=match) as e:
            ctx.call("bsc_predict_pass", family, X, ldx, yy, 9, D, W, logvar, S, *(outs or out))
        assert ("status %d:" % status) in str(e.value), str(e.value)
        ctx.sync()
        for o in out:
            assert (o.cpu().numpy() == SENTINEL).all()

    UNSUPPORTED, INVALID = -3, -1
    call("D=6", UNSUPPORTED, D=6)
    call("D=260", UNSUPPORTED, D=260)
    call("S=0", UNSUPPORTED, S=0)
    call("S=65", UNSUPPORTED, S=65)
    call("16-byte aligned", UNSUPPORTED, X=Xb.view(-1)[1:])
    call("16-byte aligned", UNSUPPORTED, W=Wb[1:])
    call("ldx=252", UNSUPPORTED, ldx=252)
    call("ldx=258", UNSUPPORTED, ldx=258)
    call("need y", INVALID, yy=None)
    call("logvar", INVALID, logvar=None)
    # the next valid call is right
    X, yv, W, logvar = _inputs("gaussian", 9, 256, 8, seed=2)
    _check(ctx, "gaussian", X, yv, W, logvar)


# ---- drivers --------------------------------------------------------------------------------------------------------

def _ar_design(n, D, seed):
    rs = np.random.RandomState(seed)
    e = rs.standard_normal((n, D))
    X = np.empty((n, D))
    X[:, 0] = e[:, 0]
    for d in range(1, D):
        X[:, d] = 0.9 * X[:, d - 1] + math.sqrt(1.0 - 0.81) * e[:, d]
    return X.astype(np.float32)


def _models(ctx, steps=0):
    """The three guides on small data, `steps` updates in."""
    from bayesic_amd.svi import GLMReparamSVI
    from bayesic_amd.svi.blr import BLRReparamSVI
    B, D = 600, 8
    X = _ar_design(B, D, 1)
    yg = (X.astype(np.float64) @ np.linspace(-1, 1, D) + 0.5 * np.random.RandomState(2).standard_normal(B)).astype(np.float32)
    yl = (yg > 0).astype(np.float32)
    out = [("glm", "logistic", GLMReparamSVI(X, yl, link="logistic", n_samples=8, seed=9, lr=0.05, ctx=ctx), X, yl),
           ("diag", "gaussian", BLRReparamSVI(X, yg, n_samples=8, seed=9, lr=0.05, ctx=ctx), X, yg),
           ("full", "gaussian", BLRReparamSVI(X, yg, n_samples=8, seed=9, lr=0.05, ctx=ctx, covariance="full"), X, yg)]
    for _, _, m, _, _ in out:
        for _ in range(steps):
            m.step()
    ctx.sync()
    return out


def test_posterior_draws_and_predict_follow_the_reference_layout(ctx):
    from bayesic_amd.svi import predict as mod
    for kind, family, m, X, y in _models(ctx, steps=5):
        for S, seed in ((64, None), (5, 77)):
            W, lv = mod.posterior_draws(m, S, seed)
            W_r, lv_r = ref.posterior_draws(kind, m.lam.cpu().numpy(), m.D, S, m.seed if seed is None else seed)
            npt.assert_array_equal(W.cpu().numpy(), W_r)
            if lv_r is None:
                assert lv is None
            else:
                npt.assert_allclose(lv.cpu().numpy(), lv_r, rtol=1e-6)   # (bitwise up to libm's exp)
            out = m.predict(X, y, n_samples=S, seed=seed)
            direct = _run(ctx, family, X, y, W.cpu().numpy(), None if lv is None else lv.cpu().numpy())
            for k in direct:
                npt.assert_array_equal(out[k].cpu().numpy(), direct[k])
            assert m.heldout_lpd(X, y, n_samples=S, seed=seed) == direct["lpd_sum"][0] / X.shape[0]
        with pytest.raises(ValueError, match="at most 64"):
            m.predict(X, n_samples=65)
        with pytest.raises(ValueError, match="columns"):
            m.predict(X[:, :4])


def test_predict_does_not_disturb_training(ctx):
    runs = []
    for with_predict in (False, True):
        state = []
        for _, _, m, X, y in _models(ctx, steps=1):
            if with_predict:
                m.predict(X, y)
            m.step()
            ctx.sync()
            state.append((m.lam.cpu().numpy().copy(), m.elbo.item(), m.grad.cpu().numpy().copy()))
        runs.append(state)
    for a, b in zip(*runs):
        npt.assert_array_equal(a[0], b[0])
        assert a[1] == b[1]
        npt.assert_array_equal(a[2], b[2])


def test_a_general_family_blr_refuses(ctx):
    from bayesic_amd.svi.blr import BLRReparamSVI
    X = _ar_design(64, 8, 1)
    m = BLRReparamSVI(X, X[:, 0].copy(), n_samples=8, ctx=ctx, family=fr.nig_family(64, 1.0, 8))
    with pytest.raises(NotImplementedError, match="precision"):
        m.predict(X)


def test_logistic_end_to_end_beats_the_prior_and_the_constant_rate(ctx):
    from bayesic_amd.svi import GLMReparamSVI
    D = 8
    X = _ar_design(3000, D, 11)
    w_true = np.random.RandomState(3).standard_normal(D)
    p = 1.0 / (1.0 + np.exp(-(X.astype(np.float64) @ w_true)))
    y = (np.random.RandomState(4).uniform(size=3000) < p).astype(np.float32)
    Xtr, ytr, Xte, yte = X[:2000], y[:2000], X[2000:], y[2000:]
    m = GLMReparamSVI(Xtr, ytr, link="logistic", n_samples=8, seed=5, lr=0.05, ctx=ctx)
    before = m.heldout_lpd(Xte, yte)
    for _ in range(300):
        m.step()
    after = m.heldout_lpd(Xte, yte)
    pbar = float(ytr.mean())
    base = float((yte * math.log(pbar) + (1 - yte) * math.log(1 - pbar)).mean())
    print("logistic held-out lpd per row: t=0 %.4f, fitted %.4f, constant rate %.4f" % (before, after, base))
    assert after > before and after > base


def test_gaussian_end_to_end_both_guides(ctx):
    from bayesic_amd.svi.blr import BLRReparamSVI
    D = 8
    X = _ar_design(3000, D, 21)
    wt = np.random.RandomState(1).standard_normal(D) / 2.0
    y = (X.astype(np.float64) @ wt + 0.5 * np.random.RandomState(2).standard_normal(3000)).astype(np.float32)
    Xtr, ytr, Xte, yte = X[:2000], y[:2000], X[2000:], y[2000:]
    v0, mu0 = float(ytr.var()), float(ytr.mean())
    base = float((-0.5 * math.log(2 * math.pi * v0) - 0.5 * (yte - mu0) ** 2 / v0).mean())
    lpd = {}
    for cov in ("diag", "full"):
        m = BLRReparamSVI(Xtr, ytr, n_samples=32, seed=5, lr=0.02, ctx=ctx, covariance=cov)
        before = m.heldout_lpd(Xte, yte)
        for _ in range(450):
            m.step()
        out = m.predict(Xte, yte)
        lpd[cov] = out["lpd"].cpu().numpy().astype(np.float64)
        after = float(out["lpd_sum"].item()) / 1000
        print("%s guide held-out lpd per row: t=0 %.4f, fitted %.4f, constant Gaussian %.4f" % (cov, before, after, base))
        assert after > before and after > base
    diff = lpd["full"] - lpd["diag"]
    se = diff.std(ddof=1) / math.sqrt(diff.size)
    print("full - mean-field: %.5f per row, standard error %.5f" % (diff.mean(), se))
    assert diff.mean() >= -se


def test_the_plugin_route_predicts_through_the_driver(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint
    from bayesic_amd.svi import GLMReparamSVI
    B, D, S, seed, lr, scale, tau = 2000, 64, 8, 21, 0.02, 7.0, 1.5
    rs = np.random.RandomState(6)
    X = ctx.to_device((rs.standard_normal((B, D)) / 8.0).astype(np.float32))
    y = ctx.to_device((rs.uniform(size=B) < 0.5).astype(np.float32))
    lj, v = logistic_regression_log_joint(scale, tau)
    lam0 = glm_ref.init_lam(D)
    eng = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx), lam0=lam0)
    assert eng.route.startswith("fused: bsc_glm"), eng.route
    hand = GLMReparamSVI(X, y, link="logistic", n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau,
                         ctx=ctx, lam0=lam0)
    for _ in range(3):
        eng.step()
        hand.step()
    a, b = eng.predict(X, y), hand.predict(X, y)
    ctx.sync()
    for k in b:
        npt.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy())
    general = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                        lam0=lam0, route="general")
    with pytest.raises(NotImplementedError, match="general"):
        general.predict(X)
