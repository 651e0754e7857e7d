"""bsc_glm_weibull_data_pass_interval on a mixed batch (events, right-, interval- and left-censored rows) against
bsc_glm_weibull_data_pass on the same rows with ``upper`` dropped, offset AND weights set on both, in one process at
1M x 256, S = 8 (rows: --rows); then one WeibullReparamSVI update with and without ``upper``.

The pass with the upper ends reads one more float per row (bytes x 1.004) and its link has seven transcendentals per
(row, draw) where the other has two; the negative-binomial pass, with a heavier link still, runs at x 1.25 of the Poisson
pass.  No target is fixed: the ratio measured here is what the README row quotes.

Method (tools/bench_glm_weibull.py's): every case runs over ROTATE copies of (X, y, upper, o, v) in turn (1 GiB of X
apiece: no copy is still in the 256 MiB Infinity Cache when its turn comes again), is warmed for at least 60 ms, and is
then timed in BLOCKS alternating blocks of REPS calls between two events on the context's stream: both sides of a ratio
share the clocks and the temperature of the minute they ran in.  Medians are reported, min and max show the block-to-block
spread.  Writes profiles/glm_weibull_interval_bench.txt (--out).

    python tools/bench_glm_weibull_interval.py [--rows N] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from bayesic_amd.svi import WeibullReparamSVI  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
PLAIN, INTERVAL = "bsc_glm_weibull_data_pass", "bsc_glm_weibull_data_pass_interval"


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_weibull_interval_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    W = 0.1 * torch.randn((S, D), generator=g, device=dev)
    logk = torch.linspace(-1.0, 1.0, S, device=dev)          # z = k (log t - l) stays small
    sets, shares = [], torch.zeros(4)
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        scale = torch.exp(X @ torch.randn(D, generator=g, device=dev) + o)
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        # Weibull(k = 1.5) durations by inversion; 40 % events, 20 % cut at a uniform fraction (right-censored), 25 % known
        # to an interval of relative width 1e-3 .. 3 below and above (one in nine with upper = 1e30), 15 % left-censored
        u = torch.rand(N, generator=g, device=dev).clamp(1e-7, 1.0 - 1e-7)
        t = (scale * (-torch.log(u)) ** (1.0 / 1.5)).clamp_min(1e-30)
        pick = torch.rand(N, generator=g, device=dev)
        cut = 0.1 + 0.9 * torch.rand(N, generator=g, device=dev)
        width = torch.exp(torch.empty(N, device=dev).uniform_(-6.9, 1.1, generator=g))
        far = torch.rand(N, generator=g, device=dev) < 1.0 / 9.0
        event, right, itv = pick < 0.4, (pick >= 0.4) & (pick < 0.6), (pick >= 0.6) & (pick < 0.85)
        left = pick >= 0.85
        lo = (t * cut).clamp_min(1e-30)
        y = torch.where(event, t, -lo)
        up = torch.where(itv, torch.where(far, torch.full_like(t, 1e30), lo * (1.0 + width)), torch.zeros_like(t))
        up = torch.where(left, -t, up)
        y = torch.where(left, -t, y)
        # the same rows with upper dropped: an interval row is right-censored at its lower end, a left-censored row at b
        sets.append(dict(X=X, o=o, v=v, y=y, u=up))
        shares += torch.tensor([event.float().mean().item(), right.float().mean().item(), itv.float().mean().item(),
                                left.float().mean().item()])
    shares = [round(float(s) / ROTATE, 4) for s in shares]
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    def pass_calls(which):
        turn = [0]

        def one():
            d = sets[turn[0] % ROTATE]
            turn[0] += 1
            if which == INTERVAL:
                ctx.call(INTERVAL, d["X"], D, d["y"], d["u"], d["o"], d["v"], N, D, W, logk, S, ell, G, T)
            else:
                ctx.call(PLAIN, d["X"], D, d["y"], d["o"], d["v"], N, D, W, logk, S, ell, G, T)
        return one

    def update_calls(model, with_upper):
        turn = [0]

        def one():
            d = sets[turn[0] % ROTATE]
            turn[0] += 1
            # raw pointers: set_batch then checks nothing and synchronises nothing
            model.set_batch(d["X"].data_ptr(), d["y"].data_ptr(), rows=N, offset=d["o"].data_ptr(),
                            weights=d["v"].data_ptr(), upper=d["u"].data_ptr() if with_upper else None)
            model.step()
        return one

    e0, e1 = ctx.event(), ctx.event()

    def block(fn, reps):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        return e0.elapsed_ms(e1)

    def compare(fns, what, floats_per_row):
        for fn in fns.values():
            elapsed = 0.0
            while elapsed < 60.0:
                elapsed += block(fn, 2 * ROTATE)
        times = {name: [] for name in fns}
        for _ in range(BLOCKS):
            for name, fn in fns.items():                      # alternating
                times[name].append(block(fn, REPS) / REPS * 1e3)
        med = {}
        for name, t in times.items():
            t.sort()
            med[name] = t[len(t) // 2]
            say({"case": "%s %s %dx%d S=%d" % (name, what, N, D, S), "us": round(med[name], 2),
                 "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                 "GBps": round(4.0 * N * (D + floats_per_row[name]) / med[name] / 1e3, 1)})
        return med

    med = compare({name: pass_calls(name) for name in (PLAIN, INTERVAL)}, "pass", {PLAIN: 3, INTERVAL: 4})
    pass_ratio = round(med[INTERVAL] / med[PLAIN], 4)

    d0 = sets[0]
    kw = dict(n_samples=S, seed=3, lr=1e-3, ctx=ctx, offset=d0["o"], weights=d0["v"])
    names = ("WeibullReparamSVI.step", "WeibullReparamSVI(upper).step")
    # the constructor takes the plain form: time (0 on a left-censored row), event, and upper with inf for "none"
    y0, u0 = d0["y"], d0["u"]
    inf = torch.full_like(y0, float("inf"))
    time = torch.where(u0 < 0, torch.zeros_like(y0), y0.abs())
    models = {names[0]: WeibullReparamSVI(d0["X"], y0.abs(), (y0 > 0) & (u0 == 0), **kw),
              names[1]: WeibullReparamSVI(d0["X"], time, (y0 > 0) & (u0 == 0),
                                          upper=torch.where(u0 > 0, u0, torch.where(u0 < 0, -u0, inf)), **kw)}
    med = compare({n: update_calls(models[n], n == names[1]) for n in names}, "update", {names[0]: 3, names[1]: 4})
    update_ratio = round(med[names[1]] / med[names[0]], 4)
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "shares_event_right_interval_left": shares,
         "pass_interval_over_plain": pass_ratio, "update_interval_over_plain": update_ratio,
         "byte_ratio": round((D + 4) / (D + 3), 4)})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_weibull_interval.py: us per call, median of %d alternating blocks of %d calls, %d "
                "rotating copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
