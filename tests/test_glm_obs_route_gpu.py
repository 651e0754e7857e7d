"""The offset / weight route of the fused GLM pass from the plugin surface (``ReparamVI`` on the builders with
``offset=True, weights=True``) and end to end on count data with exposures.

End to end (float64 reference of the same steps and draws, tests/_glm_obs_ref.py; figures from the reference alone,
recorded before the device ran): Poisson, B = 4096 training and 1024 held-out rows, D = 8, exposures log-uniform over
[0.1, 10], 60 full-batch updates at lr 0.1 with S = 8, 64 predictive draws.  Held-out log predictive density per row:
-1.6348 with the exposure as offset, -4.3732 for the model that ignores it: a gap of +2.74 per row (the two parts of
the bound below come to 1.4e-3 and 3.3e-3 per row).

The device's scores are held to the reference's by a bound made of two parts, both computed from reference quantities:
 * the predictive pass on the same draws: tests/test_predict_gpu.py's bound of lpd_sum (2e-5 (|y l| + A(l) + 1) per
   row, maximum over the draws), divided by the rows;
 * the draws themselves: the drivers are held to |lam_device - lam_reference| <= 2e-4 (the existing tolerance of the
   update tests, asserted here too), so |dw_sd| <= 2e-4 (1 + e^{rho_d} |eps_sd|), |dl_ns| <= sum_d |x_nd| |dw_sd|, and
   log p(y | l) moves by at most |y - e^l| |dl| + e^l (e^{|dl|} - 1 - |dl|); log-mean-exp is 1-Lipschitz in the
   maximum norm, so lpd_n moves by at most the maximum of that over the draws."""
import math

import numpy as np
import numpy.testing as npt
import pytest

import _glm_obs_ref as ref
import _glm_ref as glm
import _predict_ref as pred

pytestmark = pytest.mark.gpu

E2E = dict(B=4096, B_test=1024, D=8, S=8, steps=60, lr=0.1, seed=5, S_pred=64)


def exposure_data(seed=17):
    c = E2E
    n = c["B"] + c["B_test"]
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((n, c["D"])) / math.sqrt(c["D"])).astype(np.float32)
    X[:, 0] = 1.0                                               # an intercept
    expo = np.exp(rs.uniform(math.log(0.1), math.log(10.0), n)).astype(np.float32)
    w = 0.7 * rs.standard_normal(c["D"])
    y = rs.poisson(expo.astype(np.float64) * np.exp(X.astype(np.float64) @ w)).astype(np.float32)
    return X, y, expo


def reference_run(X, y, offset):
    """(lam after the steps, held-out score per row, its bound) of the float64 reference; ``offset`` or None."""
    c = E2E
    B, D = c["B"], c["D"]
    o_tr = None if offset is None else offset[:B]
    o_te = None if offset is None else offset[B:]
    lam = glm.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, c["steps"] + 1):
        lam, m1, m2, _, _ = ref.step("poisson", lam, m1, m2, t, X[:B], y[:B], c["S"], c["seed"], float(B), c["lr"],
                                     offset=o_tr)
    W, _ = pred.posterior_draws("glm", lam, D, c["S_pred"], c["seed"])
    Xte, yte = X[B:], y[B:]
    out = ref.predict("poisson", Xte, W, yte, o_te)
    bound = ref.predict_bounds("poisson", Xte, W, yte, o_te)["lpd_sum"]
    # the draws: |lam_device - lam| <= 2e-4
    eps = pred.philox.normal_draws(c["seed"], c["S_pred"], D, stream=pred.STREAM, step=0)
    dW = 2e-4 * (1.0 + np.exp(lam[D:])[None, :] * np.abs(eps))
    dl = np.abs(Xte.astype(np.float64)) @ dW.T
    mu = np.exp(ref.logits(Xte, W, o_te))
    move = np.abs(yte.astype(np.float64)[:, None] - mu) * dl + mu * (np.expm1(dl) - dl)
    bound = bound + move.max(axis=1).sum()
    return lam, out["lpd_sum"] / c["B_test"], bound / c["B_test"]


def test_end_to_end_the_exposure_model_beats_the_one_that_ignores_it(ctx):
    from bayesic_amd.svi import GLMReparamSVI
    c = E2E
    X, y, expo = exposure_data()
    B = c["B"]
    log_e = np.log(expo.astype(np.float64)).astype(np.float32)
    scores, refs = {}, {}
    for name, kw, te_kw, o in (("exposure", dict(exposure=expo[:B]), dict(exposure=expo[B:]), log_e),
                               ("ignored", {}, {}, None)):
        m = GLMReparamSVI(X[:B], y[:B], link="poisson", n_samples=c["S"], seed=c["seed"], lr=c["lr"], ctx=ctx, **kw)
        if o is not None:
            o = m.offset.cpu().numpy()
            o = np.concatenate([o, np.log(expo[B:])])     # the device's own float32 log for the training rows
        for _ in range(c["steps"]):
            m.step()
        lam_r, score_r, bound = reference_run(X, y, o)
        if o is not None:
            te_kw = dict(offset=o[B:])
        score = m.heldout_lpd(X[B:], y[B:], n_samples=c["S_pred"], **te_kw)
        drift = np.abs(m.lam.cpu().numpy() - lam_r).max()
        print("%s: held-out lpd per row %.6f, reference %.6f, |diff| %.3g, bound %.3g, lam drift %.3g"
              % (name, score, score_r, abs(score - score_r), bound, drift))
        npt.assert_allclose(m.lam.cpu().numpy(), lam_r, atol=2e-4)
        assert abs(score - score_r) <= bound, (name, score, score_r, bound)
        scores[name], refs[name] = score, score_r
    assert refs["exposure"] - refs["ignored"] > 0.0          # the reference's own gap (+2.74 per row)
    assert scores["exposure"] > scores["ignored"]


@pytest.mark.parametrize("link", ["logistic", "poisson"])
def test_the_plugin_surface_reaches_the_fused_route_with_offset_and_weights(ctx, link):
    import torch
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint, poisson_regression_log_joint
    from bayesic_amd.svi import GLMReparamSVI
    builder = logistic_regression_log_joint if link == "logistic" else poisson_regression_log_joint
    B, D, S, seed, lr, scale, tau = 1029, 64, 8, 21, 0.02, 7.0, 1.5

    def batch(k):
        rs = np.random.RandomState(k)
        X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
        o = (0.5 * rs.standard_normal(B)).astype(np.float32)
        v = rs.uniform(0.0, 2.0, B).astype(np.float32)
        v[::6] = 0.0
        L = X.astype(np.float64) @ rs.standard_normal(D) + o
        y = (rs.uniform(size=B) < 1 / (1 + np.exp(-L))) if link == "logistic" else rs.poisson(np.exp(L))
        return X, y.astype(np.float32), o, v

    X, y, o, v = batch(2)
    lj, vs = builder(scale, tau, offset=True, weights=True)
    lam0 = glm.init_lam(D)
    eng = ReparamVI(lj, [(vs["W"], D)], dict(X=X, y=y, offset=o, weights=v), n_samples=S, seed=seed, lr=lr,
                    backend=DeviceBackend(ctx), lam0=lam0)
    assert eng.route.startswith("fused") and "glm" in eng.route and eng.route_reason is None, (eng.route, eng.route_reason)
    assert eng.route == "fused: bsc_glm_data_pass + bsc_glm_update (%s link)" % link
    assert (eng.plan.offset, eng.plan.weights) == ("offset", "weights")
    hand = GLMReparamSVI(X, y, link=link, n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau,
                         ctx=ctx, lam0=lam0, offset=o, weights=v)
    for _ in range(5):
        assert eng.step() is None
        hand.step()
    ctx.sync()
    npt.assert_allclose(eng.lam, hand.lam.cpu().numpy(), rtol=1e-9, atol=1e-12)
    npt.assert_allclose(eng.elbo, hand.elbo.item(), rtol=1e-9)
    # and it is not the model without them
    plain = GLMReparamSVI(X, y, link=link, n_total=scale * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau,
                          ctx=ctx, lam0=lam0)
    for _ in range(5):
        plain.step()
    assert np.abs(plain.lam.cpu().numpy() - eng.lam).max() > 1e-3
    # set_data forwards the vectors of the next mini-batch
    X2, y2, o2, v2 = batch(3)
    eng.set_data(X=X2, y=y2, offset=o2, weights=v2)
    hand.set_batch(ctx.to_device(X2), ctx.to_device(y2), offset=ctx.to_device(o2), weights=ctx.to_device(v2))
    eng.step()
    hand.step()
    ctx.sync()
    npt.assert_allclose(eng.lam, hand.lam.cpu().numpy(), rtol=1e-9, atol=1e-12)
    # predict takes the new rows' offset and weights, and refuses to go without the offset
    with pytest.raises(ValueError, match="fitted with an offset"):
        eng.predict(X2, y2)
    out = eng.predict(X2, y2, offset=o2, weights=v2, n_samples=16)
    want = hand.predict(X2, y2, offset=o2, weights=v2, n_samples=16)
    for k in ("mean", "var", "lpd", "lpd_sum"):
        assert bool(torch.isfinite(out[k]).all())
        npt.assert_array_equal(out[k].cpu().numpy(), want[k].cpu().numpy())
