"""GPU: the full-covariance Gaussian guide of the three regression families with a learned scalar
(bsc_glm_scalar_fullrank_update; NegBinReparamSVI, GammaReparamSVI and WeibullReparamSVI with covariance="full";
posterior_draws) against the float64 restatement in tests/_glm_scalar_full_ref.py.

Tolerances (tests/test_glm_full_gpu.py's, for the same arithmetic): the finish is float64 on both sides with the same
inputs, so lam_out, m1, m2, grad and the ELBO agree to rtol 1e-10 (absolute floor 1e-10 of the largest entry, for
entries that are sums with cancellation) and the next draws within one float32 ulp; with a diagonal L the finish agrees
with bsc_glm_nb_update to 1e-12; whole driver steps take the float32 data pass and use the existing five-step tolerance
(ELBO rtol 1e-6, lam atol 1e-4)."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

from oracle import philox, svi

import _glm_scalar_full_ref as ref

pytestmark = pytest.mark.gpu

ADAM = (0.9, 0.999, 1e-8)
SCALE, PREC, A0, B0, T, LR = 12.5, 0.7, 1.3, 0.6, 3, 0.01
WHO = "bsc_glm_scalar_fullrank_update"


def _inputs(D, S, seed, offdiag=0.05):
    """Random finish inputs over P = D + 1 with non-zero off-diagonal entries, the tau row's included (offdiag = 0: a
    diagonal L).  eps and eps_next are bsc_blr_noise's [S, D + 1], every column read."""
    r = np.random.RandomState(seed)
    P = D + 1
    L = np.tril(offdiag * r.standard_normal((P, P)), -1) + np.diag(np.exp(-2.0 + 0.3 * r.standard_normal(P)))
    lam = ref.pack(0.1 * r.standard_normal(P), L)
    n = lam.size
    m1 = 0.01 * r.standard_normal(n)
    m2 = 1e-4 * r.random_sample(n)
    eps = r.standard_normal((S, P))
    W, ls = ref.draw(lam, eps)
    ell = -100.0 * r.uniform(1, 2, S)
    G = 5.0 * r.standard_normal((S, D))
    Tt = 30.0 * r.standard_normal(S)
    eps_next = r.standard_normal((S, P))
    return dict(lam=lam, m1=m1, m2=m2, eps=eps, W=W, ls=ls, ell=ell, G=G, T=Tt, eps_next=eps_next)


def _call(ctx, inp, ready=1, seed=7, next_step=4, name=WHO):
    """One finish (bsc_glm_scalar_fullrank_update, or bsc_glm_nb_update on a mean-field lam); host copies of every
    output."""
    S, D = inp["W"].shape
    dev = lambda a, dt=torch.float64: ctx.to_device(np.ascontiguousarray(a), dt)
    n = inp["lam"].size
    d = dict(stats=dev(np.concatenate([inp["ell"], inp["G"].reshape(-1), inp["T"]])), lam=dev(inp["lam"]),
             m1=dev(inp["m1"]), m2=dev(inp["m2"]), eps=dev(inp["eps"]), W=dev(inp["W"], torch.float32),
             ls=dev(inp["ls"], torch.float32),
             eps_next=dev(inp["eps_next"]) if ready else ctx.zeros((S, D + 1), torch.float64),
             W_next=ctx.zeros((S, D), torch.float32), ls_next=ctx.zeros(S, torch.float32),
             elbo=ctx.zeros(1, torch.float64), lam_out=ctx.zeros(n, torch.float64), grad=ctx.zeros(n, torch.float64))
    ctx.call(name, d["stats"], d["lam"], d["lam_out"], d["m1"], d["m2"], d["eps"], d["W"], d["ls"], D, S, SCALE, PREC,
             A0, B0, T, LR, *ADAM, seed, next_step, d["eps_next"], ready, d["W_next"], d["ls_next"], d["elbo"],
             d["grad"])
    ctx.sync()
    npt.assert_array_equal(d["lam"].cpu().numpy(), inp["lam"])            # lam_in is not modified
    out = {k: d[k].cpu().numpy() for k in ("m1", "m2", "grad", "W_next", "ls_next", "eps_next")}
    out.update(lam=d["lam_out"].cpu().numpy(), elbo=float(d["elbo"].item()))
    return out


def _finish_ref(inp):
    return ref.finish(inp["lam"], inp["m1"], inp["m2"], T, inp["eps"], inp["W"], inp["ls"], inp["ell"], inp["G"],
                      inp["T"], SCALE, PREC, A0, B0, LR)


def _close(a, b, rtol):
    b = np.asarray(b, np.float64)
    npt.assert_allclose(a, b, rtol=rtol, atol=rtol * max(np.abs(b).max(), 1e-300))


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert (np.sign(a) == np.sign(b)).all() or np.abs(a - b).max() <= np.spacing(np.abs(b)).max()
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


def _assert_next_draws(out, lam, eps_next):
    W, ls = ref.draw(lam, eps_next)
    assert _ulps(out["W_next"], W) <= 1
    assert _ulps(out["ls_next"], ls) <= 1


@pytest.mark.parametrize("S", [1, 8, 13, 64])
@pytest.mark.parametrize("D", [4, 8, 100, 256])
def test_kernel_matches_the_restatement(ctx, D, S):
    """D = 4: P = 5 and three workgroups, the smallest case with a single-row workgroup (row 2) next to two-row ones
    and the tau row (row 4) paired with row 0."""
    inp = _inputs(D, S, seed=D * 100 + S)
    out = _call(ctx, inp)
    lam, m1, m2, elbo, grad = _finish_ref(inp)
    _close(out["lam"], lam, 1e-10)
    _close(out["m1"], m1, 1e-10)
    _close(out["m2"], m2, 1e-10)
    _close(out["grad"], grad, 1e-10)
    npt.assert_allclose(out["elbo"], elbo, rtol=1e-10)
    _assert_next_draws(out, lam, inp["eps_next"])
    npt.assert_array_equal(out["eps_next"], inp["eps_next"])              # a ready eps_next is read, not drawn again


def test_kernel_draws_the_next_noise_when_it_is_not_ready(ctx):
    D, S = 100, 13
    inp = _inputs(D, S, seed=5)
    out = _call(ctx, inp, ready=0, seed=99, next_step=17)
    eps_next = ref.noise(D, S, 99, 17)                                    # [S, D + 1]: tau's column too
    npt.assert_allclose(out["eps_next"].reshape(S, D + 1), eps_next, rtol=1e-12, atol=1e-14)
    lam = _finish_ref(inp)[0]
    _close(out["lam"], lam, 1e-10)
    _assert_next_draws(out, lam, eps_next)


@pytest.mark.parametrize("D,S", [(8, 8), (256, 8), (100, 13)])
def test_diagonal_factor_reduces_to_the_mean_field_finish(ctx, D, S):
    """With every off-diagonal entry zero the ELBO, the mu / rho gradients and their Adam step are bsc_glm_nb_update's
    on the same stats."""
    P = D + 1
    inp = _inputs(D, S, seed=3, offdiag=0.0)
    out = _call(ctx, inp)
    mf_inp = dict(inp, lam=ref.to_mean_field(inp["lam"], P), m1=ref.to_mean_field(inp["m1"], P),
                  m2=ref.to_mean_field(inp["m2"], P))
    mf_out = _call(ctx, mf_inp, name="bsc_glm_nb_update")
    npt.assert_allclose(out["elbo"], mf_out["elbo"], rtol=1e-12)
    _close(ref.to_mean_field(out["grad"], P), mf_out["grad"], 1e-12)
    _close(ref.to_mean_field(out["lam"], P), mf_out["lam"], 1e-12)
    # (the next draws differ: the step gives the off-diagonal entries a gradient, so L' is no longer diagonal)


def _glm_full_grad(ctx, inp):
    """bsc_glm_fullrank_update's gradient on the w block of the same inputs: mu[:D] and rows i < D of L are the first
    D and the first D (D + 1) / 2 packed entries of the P layout."""
    S, D = inp["W"].shape
    P, nL = D + 1, D * (D + 1) // 2
    cut = lambda a: np.concatenate([a[:D], a[P:P + nL]])
    dev = lambda a, dt=torch.float64: ctx.to_device(np.ascontiguousarray(a), dt)
    lam = cut(inp["lam"])
    lam_out, grad = ctx.zeros(lam.size, torch.float64), ctx.zeros(lam.size, torch.float64)
    ctx.call("bsc_glm_fullrank_update", dev(np.concatenate([inp["ell"], inp["G"].reshape(-1)])), dev(lam), lam_out,
             dev(cut(inp["m1"])), dev(cut(inp["m2"])), dev(inp["eps"]), dev(inp["W"], torch.float32), D, S, SCALE, PREC,
             T, LR, *ADAM, 7, 4, None, 1, None, ctx.zeros(1, torch.float64), grad)
    ctx.sync()
    return grad.cpu().numpy(), cut


@pytest.mark.parametrize("D,S", [(8, 8), (100, 13)])
def test_the_w_rows_are_the_shipped_glm_full_covariance_kernels(ctx, D, S):
    """g_{s,i} for i < D does not see tau: on the same eps, W, ell and G the gradient of mu[:D] and of rows i < D of L
    is bsc_glm_fullrank_update's; T moves row D's gradient and no bit of the others."""
    inp = _inputs(D, S, seed=D + S)
    out = _call(ctx, inp)
    want, cut = _glm_full_grad(ctx, inp)
    _close(cut(out["grad"]), want, 1e-12)
    moved = _call(ctx, dict(inp, T=inp["T"] + 1.0))
    P = D + 1
    row_D = np.r_[D, P + D * (D + 1) // 2:inp["lam"].size]                # mu_D and row D of L
    rest = np.setdiff1d(np.arange(inp["lam"].size), row_D)
    assert (moved["grad"][row_D] != out["grad"][row_D]).all()
    assert moved["grad"][rest].tobytes() == out["grad"][rest].tobytes()
    assert moved["lam"][rest].tobytes() == out["lam"][rest].tobytes()


def test_two_identical_calls_give_identical_bytes(ctx):
    inp = _inputs(256, 64, seed=11)
    a, b = _call(ctx, inp), _call(ctx, inp)
    for k in ("lam", "m1", "m2", "grad", "W_next", "ls_next"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["elbo"] == b["elbo"]


def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    n = ref.n_lam(9)
    lam, m = ctx.zeros((2, n), f64), ctx.zeros((2, n), f64)
    eps, W, ls = ctx.zeros((2, 65 * 9), f64), ctx.zeros((2, 65 * 8)), ctx.zeros((2, 65))
    stats, elbo, grad = ctx.zeros(65 * 10, f64), ctx.zeros(1, f64), ctx.zeros(n, f64)

    def call(D=8, S=8, lam_out=lam[1], eps_next=eps[1], W_next=W[1], ls_in=ls[0], ls_next=ls[1], scale=1.0, prec=1.0,
             a0=1.0, b0=1.0, t=1):
        ctx.call(WHO, stats, lam[0], lam_out, m[0], m[1], eps[0], W[0], ls_in, D, S, scale, prec, a0, b0, t, 0.01,
                 *ADAM, 1, 1, eps_next, 1, W_next, ls_next, elbo, grad)

    with pytest.raises(BayesicHipError, match=WHO + ".*D=6 must be a multiple of 4"):
        call(D=6)
    with pytest.raises(BayesicHipError, match=WHO + ".*D=260"):
        call(D=260)
    with pytest.raises(BayesicHipError, match=WHO + ".*S=65"):
        call(S=65)
    with pytest.raises(BayesicHipError, match=WHO + ".*starts at 1"):
        call(t=0)
    with pytest.raises(BayesicHipError, match=WHO + ".*lam_in and lam_out must differ"):
        call(lam_out=lam[0])
    with pytest.raises(BayesicHipError, match=WHO + ".*null pointer"):
        call(ls_in=None)
    with pytest.raises(BayesicHipError, match=WHO + ".*a0=0 b0=1 must be positive"):
        call(a0=0.0)
    with pytest.raises(BayesicHipError, match=WHO + ".*a0=1 b0=-2 must be positive"):
        call(b0=-2.0)
    with pytest.raises(BayesicHipError, match=WHO + ".*scale=0 must be positive"):
        call(scale=0.0)
    with pytest.raises(BayesicHipError, match=WHO + ".*prior_precision=0 must be positive"):
        call(prec=0.0)
    with pytest.raises(BayesicHipError, match=WHO + ".*must not alias"):
        call(ls_next=ls[0])
    with pytest.raises(BayesicHipError, match=WHO + ".*all set or all null"):
        call(ls_next=None)
    ctx.sync()


# ---- the drivers -----------------------------------------------------------------------------------------------------

def _family_data(family, B=4000, D=64):
    """X of svi.make_cfg2, offsets 0.3 N(0, 1), weights U(0, 2) with every sixth exactly zero, and a response drawn from
    the family at the logits of make_cfg2's own w_true (scalar 2 for the negative binomial and the Gamma model, 1.5 and
    30 % censoring for the Weibull one).  Returns (X, the constructor's response arguments, the restatement's y, o,
    v)."""
    X, _, w_true = svi.make_cfg2(B, D)
    rs = np.random.RandomState(10)
    o = (0.3 * rs.standard_normal(B)).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    mu = np.exp(X.astype(np.float64) @ w_true + o)
    if family == "negbin":
        y = rs.negative_binomial(2, 2.0 / (2.0 + mu)).astype(np.float32)
        return X, (y,), y, o, v
    if family == "gamma":
        y = np.maximum(rs.gamma(2.0, mu / 2.0), 1e-30).astype(np.float32)
        return X, (y,), y, o, v
    t = mu * rs.weibull(1.5, B)
    event = rs.uniform(size=B) >= 0.3
    t = np.maximum(np.where(event, t, t * rs.uniform(0.1, 1.0, B)), 1e-30).astype(np.float32)
    return X, (t, event), np.where(event, t, -t).astype(np.float32), o, v


def _driver(family):
    from bayesic_amd import svi as drivers
    return {"negbin": drivers.NegBinReparamSVI, "gamma": drivers.GammaReparamSVI,
            "weibull": drivers.WeibullReparamSVI}[family]


@pytest.mark.parametrize("S", [8, 11])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_driver_five_steps_match_the_restatement(ctx, family, S):
    X, resp, y, o, v = _family_data(family)
    B, D = X.shape
    P = D + 1
    seed, lr, n_total, prec, a0, b0 = 21, 0.02, 40000.0, 1.5, 1.3, 0.7
    kw = dict(n_total=n_total, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0, b0=b0, ctx=ctx, offset=o,
              weights=v)
    model = _driver(family)(X, *resp, covariance="full", **kw)
    assert model.covariance_kind == "full"
    lam = ref.init_lam(P)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 6):
            assert model.step() is None
            lam, m1, m2, elbo, grad = ref.step(family, lam, m1, m2, t, X, y, S, seed, n_total, lr, prec, a0, b0,
                                               offset=o, weights=v)
            ctx.sync()
            print("%s S=%d t=%d: ELBO %.9g device %.9g, lam err %.3g" % (
                family, S, t, elbo, model.elbo.item(), np.abs(model.lam.cpu().numpy() - lam).max()))
            npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=1e-4)
    finally:
        ctx.call = real_call
    assert calls.count(WHO) == 5 and not [c for c in calls if c.endswith("_update") and c != WHO]
    p = model.params()
    L = p["L"]
    assert L.shape == (P, P) and (np.triu(L, 1) == 0).all() and np.abs(np.tril(L, -1)).max() > 0
    npt.assert_allclose(p["m"], lam[:P], atol=1e-4)
    npt.assert_allclose(p["rho"], np.log(np.diag(L)), rtol=1e-12, atol=1e-14)
    assert p["tau"] == (p["m"][D], p["rho"][D]) and p["w"][0].shape == (D,)
    npt.assert_allclose(model.covariance(), L @ L.T, rtol=1e-14)
    key = "phi_mean" if family == "negbin" else "shape_mean"
    npt.assert_allclose(p[key], math.exp(p["m"][D] + 0.5 * (L[D] ** 2).sum()), rtol=1e-14)
    with pytest.raises(ValueError, match="lam0 has 130 entries.*needs 2210"):
        _driver(family)(X, *resp, ctx=ctx, covariance="full", lam0=np.zeros(2 * P))


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_the_diag_keyword_is_the_driver_without_it_bit_for_bit(ctx, family):
    X, resp, y, o, v = _family_data(family)
    kw = dict(n_total=40000.0, n_samples=8, seed=21, lr=0.02, prior_precision=1.5, a0=1.3, b0=0.7, ctx=ctx, offset=o,
              weights=v)
    a, b = _driver(family)(X, *resp, **kw), _driver(family)(X, *resp, covariance="diag", **kw)
    assert a.covariance_kind == b.covariance_kind == "diag"
    for _ in range(5):
        a.step()
        b.step()
        ctx.sync()
        assert a.lam.cpu().numpy().tobytes() == b.lam.cpu().numpy().tobytes()
        assert a.elbo.item() == b.elbo.item()
        assert a.grad.cpu().numpy().tobytes() == b.grad.cpu().numpy().tobytes()
    P = X.shape[1] + 1
    npt.assert_array_equal(b.covariance(), np.diag(np.exp(2.0 * b.lam.cpu().numpy()[P:])))
    pa, pb = a.params(), b.params()
    assert sorted(pa) == sorted(pb) and "L" not in pb
    key = "phi_mean" if family == "negbin" else "shape_mean"
    assert pa[key] == pb[key] == math.exp(pb["m"][P - 1] + 0.5 * math.exp(2.0 * pb["rho"][P - 1]))


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_posterior_draws_and_the_predictive_of_a_full_model(ctx, family):
    from bayesic_amd.svi import predict as mod
    X, resp, y, _, _ = _family_data(family, B=1000, D=16)
    D = X.shape[1]
    lam0 = _inputs(D, 1, seed=2, offdiag=0.1)["lam"]
    model = _driver(family)(X, *resp, n_samples=8, seed=5, ctx=ctx, covariance="full", lam0=lam0)
    for S, seed in ((64, None), (5, 77)):
        W, ls = mod.posterior_draws(model, S, seed)
        assert W.dtype == ls.dtype == torch.float32 and tuple(W.shape) == (S, D) and tuple(ls.shape) == (S,)
        eps = philox.normal_draws(5 if seed is None else seed, S, D + 1, stream=mod.PREDICT_STREAM, step=0)
        W_r, ls_r = ref.draw(lam0, eps)
        assert _ulps(W.cpu().numpy(), W_r) <= 1
        assert _ulps(ls.cpu().numpy(), ls_r) <= 1
    out = model.predict(X, *resp, n_samples=16)
    for k in ("mean", "var", "lpd"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert math.isfinite(model.heldout_lpd(X, *resp, n_samples=16))
    if family == "weibull":
        surv = model.survival(X, resp[0], n_samples=16)
        assert bool(((surv >= 0) & (surv <= 1)).all())


def posterior_covariance_errors(ctx, seed, steps=4000, D=8, B=2000, S=8, lr=1e-2):
    """Relative Frobenius error of the 9 x 9 Cov_q over [w | tau] (averaged over the second half of the steps) against
    the Laplace covariance at the MAP: (full guide, mean-field guide)."""
    from bayesic_amd.svi import WeibullReparamSVI
    X, y = ref.ar_weibull_design(B, D, seed)
    _, exact = ref.laplace("weibull", X, y, prec=1.0, a0=1.0, b0=0.1)
    errs = []
    for cov in ("full", "diag"):
        model = WeibullReparamSVI(X, np.abs(y), y > 0, n_samples=S, seed=seed, lr=lr, ctx=ctx, covariance=cov)
        acc = np.zeros((D + 1, D + 1))
        for t in range(1, steps + 1):
            model.step()
            if t > steps // 2:
                acc += model.covariance()
        errs.append(ref.covariance_error(acc / (steps - steps // 2), exact))
    return tuple(errs)


def test_full_guide_recovers_the_correlated_posterior_covariance(ctx):
    """Weibull, D = 8 (an intercept column followed by seven AR(0.9) features), B = 2000, about 30 % of the rows
    right-censored, prior precision 1, Gamma(1, 0.1) prior of the shape, S = 8, 4000 steps of lr 1e-2 (seed 1), L L^T
    averaged over the second half, against the Laplace covariance of [w | tau] at the MAP: the full guide's 9 x 9
    covariance is close to it, the mean-field guide's is not.

    The float64 numpy restatement on the same Philox draws measures full 0.059 and mean-field 0.923
    (tests/test_glm_scalar_full_cpu.py), inside the condition on the reference (full <= 0.075, mean-field >= 0.75); the
    device's own figures are printed by this test: full 0.0591 and mean-field 0.9232 on one MI355X.  The thresholds are
    tests/test_glm_full_gpu.py's."""
    full, diag = posterior_covariance_errors(ctx, seed=1)
    print("full %.4f mean-field %.4f" % (full, diag))
    assert full <= 0.15, full
    assert diag >= 0.5, diag
