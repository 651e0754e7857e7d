"""The C-ABI calls of the seven reparameterised drivers, written down by tests/_trace_ctx.TraceContext and compared with
tests/golden/reparam_driver_traces.json (the negative-binomial cases: reparam_driver_traces_negbin.json; the Gamma and
Weibull drivers and the full guide of the three learned-scalar drivers: reparam_driver_traces_scalar.json): for every
case the names, scalar arguments, buffers (and which half of each
double buffer) and reserve sizes of construction, posterior_draws, three steps, set_batch with tensors, a step,
set_batch with raw pointers and one more step; with SHA-256 digests of the start lam, of the first draw (W, and xi, Bz
logphi or logshape where the driver has them) and of the predictive draws, all of which the drivers compute on the host.
Equality, not closeness: the drivers' numerics are pinned on the device by the GPU tests, and this shows that the same
calls reach the library.

``python tests/test_reparam_driver_trace_cpu.py`` writes the golden files from the tree it runs in.
"""
import json
import os

import numpy as np
import pytest
import torch

from _trace_ctx import TraceContext

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reparam_driver_traces.json")
# the negative-binomial cases came later and have a file of their own: the first one stays as it was, byte for byte
GOLDEN_NEGBIN = GOLDEN[:-5] + "_negbin.json"
# ... and so have the cases that pin the three learned-scalar drivers as a group
GOLDEN_SCALAR = GOLDEN[:-5] + "_scalar.json"
B, D, J, K, B2, LD2 = 40, 12, 5, 3, 24, 16
RAW = dict(X=0x10000, y=0x20000, offset=0x30000, weights=0x40000, groups=0x50000, upper=0x60000)


def _full_lam0(P, seed):
    """A full-layout start with a dense factor, so that the first draw goes through every entry of L."""
    rs = np.random.RandomState(seed)
    return 0.3 * rs.standard_normal(P + P * (P + 1) // 2)


def _batch(rows, seed, ld=D):
    rs = np.random.RandomState(seed)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    out = dict(X=f32(rs.standard_normal((rows, ld)))[:, :D], y=f32(rs.poisson(1.5, rows)),
               labels=torch.from_numpy(rs.randint(K, size=rows).astype(np.int32)),
               groups=torch.from_numpy(rs.randint(J, size=rows).astype(np.int32)),
               offset=f32(0.1 * rs.standard_normal(rows)), exposure=f32(rs.uniform(0.5, 2.0, rows)),
               weights=f32(rs.uniform(0.0, 3.0, rows)))
    # the learned-scalar drivers' vectors, drawn after the ones above: a strictly positive response, the censoring flags,
    # and upper ends of every kind (0: none, inf; 1: an interval above the time; 2: left-censored, the time is 0)
    pos = rs.gamma(2.0, 1.0, rows) + 0.05
    event = rs.randint(2, size=rows).astype(bool)
    kind = rs.randint(3, size=rows)
    kind[:3] = (0, 1, 2)
    upper = np.where(kind == 0, np.inf, np.where(kind == 1, pos * rs.uniform(1.5, 3.0, rows), rs.uniform(0.5, 2.0, rows)))
    out.update(ypos=f32(pos), event=torch.from_numpy(event), time0=f32(np.where(kind == 2, 0.0, pos)), upper=f32(upper))
    return out


def _blr(**kw):
    from bayesic_amd.svi.blr import BLRReparamSVI
    return BLRReparamSVI, ("X", "y"), kw, ()


def _glm(obs=(), **kw):
    from bayesic_amd.svi import GLMReparamSVI
    return GLMReparamSVI, ("X", "y"), kw, obs


def _softmax(**kw):
    from bayesic_amd.svi import SoftmaxReparamSVI
    return SoftmaxReparamSVI, ("X", "labels"), dict(kw, n_classes=K), ()


def _hier(obs=(), **kw):
    from bayesic_amd.svi import HierGLMReparamSVI
    return HierGLMReparamSVI, ("X", "y", "groups"), dict(kw, n_groups=J), obs


def _negbin(obs=(), **kw):
    from bayesic_amd.svi import NegBinReparamSVI
    return NegBinReparamSVI, ("X", "y"), kw, obs


def _gamma(obs=(), **kw):
    from bayesic_amd.svi import GammaReparamSVI
    return GammaReparamSVI, ("X", "ypos"), kw, obs


def _weibull(obs=(), time="ypos", **kw):
    """(X, time, event) are the constructor's first three; with ``upper`` the time has its zeros and event is None."""
    from bayesic_amd.svi import WeibullReparamSVI
    return WeibullReparamSVI, ("X", time) + (() if "upper" in obs else ("event",)), kw, obs


CASES = {
    "blr-diag-S8": lambda: _blr(n_samples=8),
    "blr-diag-S16": lambda: _blr(n_samples=16),
    "blr-full": lambda: _blr(covariance="full", lam0=_full_lam0(D + 1, 1)),
    "blr-family": lambda: _blr(family=(0.5, -1.5, 2.0, 1.0, 0.25)),
    "blr-reproducible": lambda: _blr(reproducible=True),
    "blr-stream": lambda: _blr(sweep="stream"),
    "glm-logistic-S8": lambda: _glm(link="logistic", n_samples=8),
    "glm-logistic-S16": lambda: _glm(link="logistic", n_samples=16),
    "glm-full": lambda: _glm(link="logistic", covariance="full", lam0=_full_lam0(D, 2)),
    "glm-poisson-exposure-weights": lambda: _glm(("exposure", "weights"), link="poisson"),
    "glm-logistic-offset": lambda: _glm(("offset",), link="logistic"),
    "softmax-diag": lambda: _softmax(),
    "softmax-full": lambda: _softmax(covariance="full", lam0=_full_lam0(K * D, 3)),
    "hier-S8": lambda: _hier(n_samples=8),
    "hier-S12": lambda: _hier(n_samples=12),
    "hier-offset-weights": lambda: _hier(("offset", "weights")),
    "negbin-S8": lambda: _negbin(n_samples=8),
    "negbin-S12": lambda: _negbin(n_samples=12),
    "negbin-exposure-weights": lambda: _negbin(("exposure", "weights")),
}
SCALAR_CASES = {
    "gamma-S8": lambda: _gamma(n_samples=8),
    "gamma-exposure-weights": lambda: _gamma(("exposure", "weights")),
    "gamma-full": lambda: _gamma(covariance="full", lam0=_full_lam0(D + 1, 4)),
    "negbin-full": lambda: _negbin(covariance="full", lam0=_full_lam0(D + 1, 5)),
    "weibull-S8": lambda: _weibull(n_samples=8),
    "weibull-S12": lambda: _weibull(n_samples=12),
    "weibull-offset-weights": lambda: _weibull(("offset", "weights")),
    "weibull-upper": lambda: _weibull(("upper",), time="time0"),
    "weibull-upper-offset-weights": lambda: _weibull(("upper", "offset", "weights"), time="time0"),
    "weibull-full": lambda: _weibull(covariance="full", lam0=_full_lam0(D + 1, 6)),
}
CASES.update(SCALAR_CASES)


def record(case):
    from bayesic_amd.svi.predict import posterior_draws
    cls, positional, kw, obs = CASES[case]()
    ctx = TraceContext()
    # (the reproducible mode keeps its shards of the first batch's rows: its next batch has as many)
    first, second = _batch(B, 11), _batch(B if kw.get("reproducible") else B2, 12, LD2)
    ctx.name(**first)
    model = cls(*(first[k] for k in positional), n_total=400.0, seed=77, lr=0.02, ctx=ctx,
                **dict(kw, **{k: first[k] for k in obs}))
    ctx.bind(model)
    ctx.digest("_lam", model._lam)
    if cls.__name__ != "HierGLMReparamSVI" and "family" not in kw:      # the two that have no predictive
        for label, t in zip(("draws W", "draws logvar"), posterior_draws(model, 8)):
            if t is not None:
                ctx.digest(label, t)
        ctx.bind(model)
    model.step()
    ctx.bind(model)
    for attr in ("_W", "_xi", "_Bz", "_logphi", "_logshape"):
        if hasattr(model, attr):
            ctx.digest(attr, getattr(model, attr))
    model.step()
    model.step()
    ctx.bind(model)
    # the next batch: tensors (exposure is a constructor argument; a batch brings its offset)
    extra = ["offset" if k == "exposure" else k for k in obs] + list(positional[2:])
    ctx.name(**{k + "2": v for k, v in second.items()})
    model.set_batch(*(second[k] for k in positional[:2]), **{k: second[k] for k in extra})
    model.step()
    ctx.bind(model)
    if not kw.get("reproducible"):          # (that mode cuts tensors into shards and refuses raw pointers)
        # (Weibull: y is the signed vector and upper the device encoding; event= is for tensors)
        model.set_batch(RAW["X"], RAW["y"], rows=B2, ldx=LD2, **{k: RAW[k] for k in extra if k != "event"})
        model.step()
        ctx.bind(model)
    return json.loads(json.dumps(ctx.trace))


@pytest.fixture(scope="module")
def golden():
    traces = {}
    for path in (GOLDEN, GOLDEN_NEGBIN, GOLDEN_SCALAR):
        with open(path) as f:
            traces.update(json.load(f))
    return traces


def test_every_case_has_a_recorded_trace(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_driver_makes_the_recorded_calls(case, golden):
    got, want = record(case), golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "event %d" % i
    assert len(got) == len(want)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    file_of = lambda case: GOLDEN_SCALAR if case in SCALAR_CASES else \
        GOLDEN_NEGBIN if case.startswith("negbin-") else GOLDEN
    for path in (GOLDEN, GOLDEN_NEGBIN, GOLDEN_SCALAR):
        mine = [case for case in sorted(CASES) if file_of(case) == path]
        with open(path, "w") as f:
            json.dump({case: record(case) for case in mine}, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
