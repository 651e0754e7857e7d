"""One update with covariance="full" against one with covariance="diag" for NegBinReparamSVI, GammaReparamSVI and
WeibullReparamSVI, in one process at 1M x 256, S = 8 (rows: --rows), offset AND weights set; then the finish on its own
through the context's profiling slot 2: glm_scalar_fullrank_update_kernel (one launch, P = 257: 129 workgroups) against
the two launches of the mean-field finish.  The pass, the all-reduce and the batch are the same on both sides, so the
whole difference of an update is the finish.

The project's own yardsticks to read the result against: blr_fullrank_update_kernel takes 8.4 us mean at P = 257 and the
whole update there is x1.025 the mean-field one (tools/bench_fullrank.py); the mean-field route of these families pays
two finish launches, about 10 us between the 176 us pass and the 186 us update (tools/bench_glm_nb.py).

Method (tools/bench_glm_weibull.py's): every case runs over ROTATE copies of (X, y, o, v) in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then
timed launch to launch in BLOCKS blocks of REPS calls between two events.  The two guides of a family alternate block
by block, so drift of the clocks or of a shared machine falls on both.  A line reports the median block and the min-max
spread.  The finish is then timed with the context's events around it (profiling on, slot 2) over PROFILED updates of
each model: the mean per update, both launches together on the mean-field side.  Results go to stdout and to
profiles/glm_scalar_full_bench.txt (--out).

    python tools/bench_glm_scalar_full.py [--rows N] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from bayesic_amd.svi import GammaReparamSVI, NegBinReparamSVI, WeibullReparamSVI  # noqa: E402

BLOCKS, REPS, ROTATE, PROFILED = 9, 20, 2, 200
FAMILIES = ("negbin", "gamma", "weibull")


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_scalar_full_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        mu = torch.exp(X @ torch.randn(D, generator=g, device=dev) + o)
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        # Weibull(k = 1.5) durations by inversion; 30 % of the rows cut at a uniform fraction and flagged by the sign
        u = torch.rand(N, generator=g, device=dev).clamp(1e-7, 1.0 - 1e-7)
        t = (mu * (-torch.log(u)) ** (1.0 / 1.5)).clamp_min(1e-30)
        cens = torch.rand(N, generator=g, device=dev) < 0.3
        cut = 0.1 + 0.9 * torch.rand(N, generator=g, device=dev)
        sets.append(dict(X=X, o=o, v=v, negbin=torch.poisson(mu * 2.0 * torch.rand(N, generator=g, device=dev)),
                         gamma=t, weibull=torch.where(cens, -(t * cut).clamp_min(1e-30), t)))
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    def update_calls(model, key):
        turn = [0]

        def one():
            d = sets[turn[0] % ROTATE]
            turn[0] += 1
            # raw pointers: set_batch then checks nothing and synchronises nothing
            model.set_batch(d["X"].data_ptr(), d[key].data_ptr(), rows=N, offset=d["o"].data_ptr(),
                            weights=d["v"].data_ptr())
            model.step()
        return one

    e0, e1 = ctx.event(), ctx.event()

    def block(fn, reps):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        return e0.elapsed_ms(e1)

    def compare(fns, what):
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
                 "us_min": round(t[0], 2), "us_max": round(t[-1], 2)})
        return med

    d0 = sets[0]
    kw = dict(n_samples=S, seed=3, lr=1e-3, ctx=ctx, offset=d0["o"], weights=d0["v"])

    def build(family, cov):
        if family == "negbin":
            return NegBinReparamSVI(d0["X"], d0["negbin"], covariance=cov, **kw)
        if family == "gamma":
            return GammaReparamSVI(d0["X"], d0["gamma"], covariance=cov, **kw)
        return WeibullReparamSVI(d0["X"], d0["weibull"].abs(), d0["weibull"] > 0, covariance=cov, **kw)

    summary = {}
    for family in FAMILIES:
        models = {cov: build(family, cov) for cov in ("diag", "full")}
        fns = {"%s(%s).step" % (family, cov): update_calls(m, family) for cov, m in models.items()}
        med = compare(fns, "update")
        ctx.sync()
        ctx.profile(1)
        finish = {}
        for (name, fn), cov in zip(fns.items(), models):
            ctx.profile_read(2)                               # drop what the slot holds
            for _ in range(PROFILED):
                fn()
            ms, launches = ctx.profile_read(2)
            finish[cov] = ms / PROFILED * 1e3
            say({"case": "%s finish (profiling slot 2)" % name, "us_per_update": round(finish[cov], 2),
                 "timed_scopes": launches, "updates": PROFILED})
        ctx.profile(0)
        ratio = med["%s(full).step" % family] / med["%s(diag).step" % family]
        summary[family] = {"update_full_over_diag": round(ratio, 4), "finish_full_us": round(finish["full"], 2),
                           "finish_diag_us": round(finish["diag"], 2)}
        del models, fns
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "P": D + 1, "lam_entries_full": D + 1 + (D + 1) * (D + 2) // 2, **summary})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_scalar_full.py: us per update, median of %d alternating blocks of %d updates, %d "
                "rotating copies of the operands; the finish from the context's events, mean of %d updates\n"
                % (BLOCKS, REPS, ROTATE, PROFILED))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
