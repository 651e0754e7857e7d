"""The VI engines with latents declared float64 -- alone, over float32 data, and with everything float64 -- on every
route, against the host engines in float64 (backend=NumpyBackend(np.float64)) on the device's own draws.

Three defects of this kind were silent before these tests: the resident pass route handed a float64 W block to
bsc_blr_data_pass_sweep, which reads float32 W [S, D] (the ELBO came out -inf, no error); the resident general route
gathered the gradients of several latents in a float32 buffer; and ScoreFunctionVI rounded every latent to float32
before upload, so a float64 model could not match its float64 twin past float32 precision.

Tolerances.  Over float32 data the data term is float32 work on every device route (the fused pass reads float32 W and
X; the general route contracts float32 X), so the pass-route tests' bounds apply: 2e-6 relative on the ELBO, 2e-5 of
the largest gradient entry, 2e-4 absolute on lam after the Adam steps.  With everything float64 no step is float32:
1e-10 relative on the ELBO, 1e-10 of the largest gradient entry (control-variate and pathwise gradients are means of
products of O(1e4) log-joint values: their rounding is ~1e-12 of the scale, one float32 rounding ~6e-8) and 1e-10 on
lam.  (The resident general route once gathered the gradients of several latents in a float32 buffer: 2e-8.)"""
import math

import numpy as np
import numpy.testing as npt
import pytest

from oracle import svi
from oracle.einsum_eval import NumpyBackend

pytestmark = pytest.mark.gpu


def _known_noise_model(two_latents, dtype):
    """test_plugin_route_gpu.test_pass_route_with_its_state_on_the_device's model with the latents declared `dtype`."""
    from bayesic_amd import algebra as A
    D = 24
    X, y = A.var("X", 2), A.var("y", 1)
    W, c = A.var("W", 2, dtype), A.var("c", 2, dtype)
    r = A.dimshuffle(y, "x", 0) - A.dot(W, X.T)
    lj = A.sum(r * r, axis=1) * (-0.5 / 0.25) + A.sum(W * W, axis=1) * (-0.5)
    latents = [(W, D)]
    if two_latents:
        lj = lj + A.sum(c * c, axis=1) * (-0.005)
        latents.append((c, 1))
    return lj, latents


def _data(N=30000, D=24):
    rs = np.random.RandomState(14)
    Xs = rs.standard_normal((N, D)).astype(np.float32)
    ys = (Xs @ (rs.standard_normal(D) / 4) + 0.5 * rs.standard_normal(N)).astype(np.float32)
    return Xs, ys


VARIANTS = [("pass", dict(resident=False)), ("pass, resident", dict(resident=True)),
            ("general, resident", dict(route="general", resident=True)),
            ("general, graph", dict(route="general", resident=False, graph=True)),
            ("general", dict(route="general", resident=False))]


@pytest.mark.parametrize("two_latents", [False, True])
@pytest.mark.parametrize("name,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_float64_latents_over_float32_data_match_the_float64_host_engine(ctx, name, kw, two_latents):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    S, seed, lr = 8, 9, 0.02
    lj, latents = _known_noise_model(two_latents, "float64")
    Xs, ys = _data()
    eng = ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx), **kw)
    assert eng.route.startswith(name.split(",")[0]), eng.route
    assert ("resident" in eng.route) == ("resident" in name), eng.route
    probe = ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, seed=seed, backend=DeviceBackend(ctx),
                      route="general", resident=False)
    host = ReparamVI(lj, latents, dict(X=Xs, y=ys), n_samples=S, seed=seed, lr=lr, backend=NumpyBackend(np.float64),
                     noise=probe.draw)
    for step in range(8):
        want = host.step()
        eng.step()
        assert abs(eng.elbo - want) <= 2e-6 * abs(want), (name, step, eng.elbo, want)
        scale = np.abs(host.grad).max()
        assert np.abs(eng.grad - host.grad).max() <= 2e-5 * scale, (name, step, np.abs(eng.grad - host.grad).max(), scale)
    npt.assert_allclose(eng.lam, host.lam, rtol=0, atol=2e-4)


@pytest.mark.parametrize("resident", [False, True])
def test_everything_float64_takes_the_general_route_at_float64_accuracy(ctx, resident):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import linear_regression_log_joint
    B, D, S, seed, lr = 4000, 16, 8, 21, 0.01
    X, y, _ = svi.make_cfg2(B, D)
    X, y = X.astype(np.float64), y.astype(np.float64)
    lj, v = linear_regression_log_joint(5.0, 1.0, 1.0, dtype="float64")
    latents = [(v["W"], D), (v["xi"], 1)]
    eng = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx),
                    resident=resident)
    assert eng.route.startswith("general"), eng.route
    assert "float32 data" in eng.route_reason, eng.route_reason          # the fused pass wants float32 X, y
    host = ReparamVI(lj, latents, dict(X=X, y=y), n_samples=S, seed=seed, lr=lr, backend=NumpyBackend(np.float64),
                     noise=eng.draw)
    for step in range(6):
        want = host.step()
        eng.step()
        assert abs(eng.elbo - want) <= 1e-10 * abs(want), (step, eng.elbo, want)
        scale = np.abs(host.grad).max()
        assert np.abs(eng.grad - host.grad).max() <= 1e-10 * scale, (step, np.abs(eng.grad - host.grad).max(), scale)
    npt.assert_allclose(eng.lam, host.lam, rtol=0, atol=1e-10)


def _config5_expression(D, G, scale, a0, b0, dtype):
    """test_plugin_route_gpu._config5_expression with every input declared `dtype`."""
    from bayesic_amd import algebra as A
    Xv, yv, Gm = A.var("X", 2, dtype), A.var("y", 1, dtype), A.var("Gm", 2, dtype)
    W, Bg, Z = A.var("W", 2, dtype), A.var("Bg", 2, dtype), A.var("Z", 2, dtype)
    L = A.dot(Xv, W.T) + A.dot(Gm, Bg.T)
    loglik = A.sum(A.dimshuffle(yv, 0, "x") * L - A.log(1 + A.exp(L)), axis=0)
    zeta = A.sum(Z, axis=1)
    lp_w = A.sum(-0.5 * (W * W), axis=1) - 0.5 * D * math.log(2 * math.pi)
    lp_b = (-0.5 * G * math.log(2 * math.pi)) + (0.5 * G) * zeta - 0.5 * (A.exp(zeta) * A.sum(Bg * Bg, axis=1))
    lp_z = (a0 * math.log(b0) - math.lgamma(a0)) + a0 * zeta - b0 * A.exp(zeta)
    return scale * loglik + lp_w + lp_b + lp_z, [(W, D), (Bg, G), (Z, 1)]


@pytest.mark.parametrize("graph", [False, True])
def test_score_function_engine_in_float64_matches_its_host_twin(ctx, graph):
    """ScoreFunctionVI draws on the device and steps on the host; its host twin evaluates the log-joint with the
    float64 numpy oracle instead of the executor, on the same draws -- the estimators and Adam are the same code."""
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ScoreFunctionVI
    N, D, G, S, seed, lr = 3000, 16, 7, 64, 5, 0.05
    X, y, g, _, _ = svi.make_cfg5(N, D, G)
    lj, latents = _config5_expression(D, G, 10.0, 1.0, 1.0, "float64")
    data = {"X": X.astype(np.float64), "y": y.astype(np.float64), "Gm": np.eye(G)[g]}
    eng = ScoreFunctionVI(lj, latents, data, n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx), graph=graph)
    assert eng.route == "general", (eng.route, eng.route_reason)         # (the fused pass streams float32 data)
    host_fn = lj.compile(NumpyBackend(np.float64))

    class HostTwin(ScoreFunctionVI):
        def log_joint_values(self, z):
            inputs, offset = dict(data), 0
            for v, n in self.latents:
                inputs[v.name] = z[:, offset:offset + n]
                offset += n
            return np.asarray(host_fn(**inputs), np.float64).reshape(self.S)

    host = HostTwin(lj, latents, data, n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx), route="general")
    for step in range(4):
        want = host.step()
        eng.step()
        assert abs(eng.elbo - want) <= 1e-10 * abs(want), (step, eng.elbo, want)
        npt.assert_allclose(eng.f, host.f, rtol=1e-11, atol=0)
        scale = np.abs(host.grad).max()
        assert np.abs(eng.grad - host.grad).max() <= 1e-10 * scale, (step, np.abs(eng.grad - host.grad).max(), scale)
    npt.assert_allclose(eng.lam, host.lam, rtol=0, atol=1e-10)
