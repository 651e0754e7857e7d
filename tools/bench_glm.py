"""The fused GLM route against the pass it was modelled on and the route it replaces, in one process at
1M x 256, S = 8 (rows: --rows).  Each case is warmed for at least 60 ms of back-to-back calls (a kernel reaches its
steady rate only after ~35 ms of continuous running) and then timed in BLOCKS blocks of REPS calls between two
events; a line reports the median block and the min-max spread:

  (a) bsc_blr_data_pass on the default route        (the HBM-bound yardstick: the same bytes per row)
  (b) bsc_glm_data_pass, logistic and Poisson        ((b) / (a) is the figure of merit)
  (c) a GLMReparamSVI update, both links             (pass + fused finish)
  (e) a GLMReparamSVI(covariance="full") update, both links (pass + slab reduce + bsc_glm_fullrank_update), with
      the finish kernel's own time (bsc_ctx_profile slot 2) -- next to (c), and next to
  (f) ReparamVI(guide="full", route="general") on the logistic log-joint: the same guide stepped on the host
  (d) ReparamVI(route="general") on the logistic log-joint: what the same model cost before the fused route

    python tools/bench_glm.py [--rows N] [--json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

BLOCKS, REPS = 7, 20
HBM_PEAK_GBS = 8000.0


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(ctx, fn, reps=REPS, warm_ms=60.0):
    """us per call: (median, min, max) over BLOCKS blocks of `reps` calls."""
    e0, e1 = ctx.event(), ctx.event()
    elapsed = 0.0
    while elapsed < warm_ms:
        e0.record()
        fn()
        fn()
        e1.record()
        elapsed += e0.elapsed_ms(e1)
    blocks = []
    for _ in range(BLOCKS):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        blocks.append(e0.elapsed_ms(e1) / reps * 1e3)
    blocks.sort()
    return blocks[len(blocks) // 2], blocks[0], blocks[-1]


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, D), generator=g, device=dev) / 16.0                 # logits of unit scale for unit-scale draws
    w_true = torch.randn(D, generator=g, device=dev)
    logits = X @ w_true
    y_gauss = logits + 0.5 * torch.randn(N, generator=g, device=dev)
    y_bern = (torch.rand(N, generator=g, device=dev) < torch.sigmoid(logits)).to(torch.float32)
    y_pois = torch.poisson(torch.exp(logits), generator=g)
    W = 0.1 * torch.randn((S, D), generator=g, device=dev)
    out_s, out_g = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    bytes_per_pass = 4.0 * N * (D + 1)
    results = []

    def report(label, t, passes=1):
        med, lo, hi = t
        line = {"case": label, "us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}
        if passes:
            line["GBps"] = round(passes * bytes_per_pass / med / 1e3, 1)
            line["fraction_of_hbm_peak"] = round(passes * bytes_per_pass / med / 1e3 / HBM_PEAK_GBS, 3)
        results.append(line)
        print(json.dumps(line), flush=True)

    t_a = timed(ctx, lambda: ctx.call("bsc_blr_data_pass", X, D, y_gauss, N, D, W, S, out_s, out_g))
    report("(a) bsc_blr_data_pass %dx%d S=%d" % (N, D, S), t_a)
    t_b = {}
    for code, link, y in ((0, "logistic", y_bern), (1, "poisson", y_pois)):
        t_b[link] = timed(ctx, lambda: ctx.call("bsc_glm_data_pass", code, X, D, y, N, D, W, S, out_s, out_g))
        report("(b) bsc_glm_data_pass %s" % link, t_b[link])

    from bayesic_amd.svi import GLMReparamSVI
    t_c = {}
    for link, y in (("logistic", y_bern), ("poisson", y_pois)):
        model = GLMReparamSVI(X, y, link=link, n_total=10.0 * N, n_samples=S, seed=1, lr=1e-3, ctx=ctx)
        t_c[link] = timed(ctx, model.step)
        report("(c) GLMReparamSVI.step %s" % link, t_c[link])
        del model

    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.inference.models import logistic_regression_log_joint
    lj, v = logistic_regression_log_joint(10.0, 1.0)

    t_e = {}
    for link, y in (("logistic", y_bern), ("poisson", y_pois)):
        model = GLMReparamSVI(X, y, link=link, n_total=10.0 * N, n_samples=S, seed=1, lr=1e-3, ctx=ctx,
                              covariance="full")
        t_e[link] = timed(ctx, model.step)
        report("(e) GLMReparamSVI(covariance='full').step %s" % link, t_e[link])
        ctx.profile(1)                      # the finish kernel alone: event pairs around its launch (slot 2)
        ctx.profile_read(2)
        for _ in range(50):
            model.step()
        ms, cnt = ctx.profile_read(2)
        ctx.profile(0)
        line = {"case": "(e) glm_fullrank_update_kernel %s D=%d S=%d" % (link, D, S),
                "us_mean": round(ms / max(cnt, 1) * 1e3, 2), "launches": cnt,
                "beside": "blr_fullrank_update_kernel: 8.4 us mean (profiles/fullrank_kernel_stats.csv)"}
        results.append(line)
        print(json.dumps(line), flush=True)
        del model
    full_general = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y_bern), n_samples=S, seed=1, lr=1e-3,
                             backend=DeviceBackend(ctx), route="general", guide="full")
    assert full_general.route.startswith("general"), full_general.route
    t_f = timed(ctx, full_general.step, reps=3, warm_ms=10.0)
    report("(f) ReparamVI(guide='full', route='general').step logistic", t_f, passes=0)
    del full_general
    eng = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y_bern), n_samples=S, seed=1, lr=1e-3, backend=DeviceBackend(ctx),
                    route="general", resident=True)
    assert eng.route.startswith("general"), eng.route
    t_d = timed(ctx, eng.step, reps=5, warm_ms=30.0)
    report("(d) ReparamVI(route='general', resident=True).step logistic", t_d, passes=0)
    auto = ReparamVI(lj, [(v["W"], D)], dict(X=X, y=y_bern), n_samples=S, seed=1, lr=1e-3, backend=DeviceBackend(ctx))
    assert auto.route.startswith("fused"), auto.route
    report("(c') ReparamVI(route='auto').step logistic: %s" % auto.route, timed(ctx, auto.step))
    ctx.sync()

    spread_a = (t_a[2] - t_a[1]) / t_a[0]
    summary = {"rows": N, "D": D, "S": S,
               "b_over_a": {k: round(t_b[k][0] / t_a[0], 3) for k in t_b},
               "spread_of_a": round(spread_a, 3),
               "c_over_d": {k: round(t_c[k][0] / t_d[0], 3) for k in t_c},
               "e_over_c": {k: round(t_e[k][0] / t_c[k][0], 3) for k in t_e},
               "e_over_f": {k: round(t_e[k][0] / t_f[0], 3) for k in t_e},
               "c_faster_than_d": all(t_c[k][0] < t_d[0] for k in t_c)}
    print(json.dumps(summary), flush=True)
    if not summary["c_faster_than_d"]:
        sys.exit("the fused GLM update is not faster than the general route it replaces")


if __name__ == "__main__":
    main()
