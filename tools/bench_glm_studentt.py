"""bsc_glm_studentt_data_pass against bsc_glm_data_pass_obs with the Poisson link and bsc_glm_lognormal_data_pass, offset AND
weights set on all three, in one process at 1M x 256, S = 8 (rows: --rows); then one StudentTReparamSVI update against one
GLMReparamSVI(link="poisson") and one LogNormalReparamSVI update on the same rows.  The passes read the same bytes,
4 D + 12 per row (the eight tau are 32 bytes per launch, the degrees of freedom one kernel argument): the byte ratio is
1.000.  No target is fixed in advance.  The Student-t link has one log, one division and one reciprocal per (row, draw)
where the Poisson link has one exp and the log-normal link one log, one exp, one more log, a degree-11 polynomial and
three reciprocals; from the instruction count it should sit near the Gamma pass, a few per cent above the Poisson pass.

Method (tools/bench_glm_lognormal.py's): every case runs over ROTATE copies of (X, y, o, v) in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then
timed launch to launch in BLOCKS blocks of REPS calls between two events.  The sides alternate block by block, so
drift of the clocks or of a shared machine falls on all of them.  A line reports the median block and the min-max
spread.  The Poisson side reads positive durations (as rates), the log-normal side the same durations with about 30 % of
the rows censored (cut at a uniform fraction, sign flipped), the Student-t side their location plus noise of sd 0.7, a
tenth of the rows with the noise times 20, at df = 4.  Results go to stdout and to profiles/glm_studentt_bench.txt (--out).

    python tools/bench_glm_studentt.py [--rows N] [--df NU] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from bayesic_amd.svi import GLMReparamSVI, LogNormalReparamSVI, StudentTReparamSVI  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
POISSON, LOGNORMAL = "bsc_glm_data_pass_obs(poisson)", "bsc_glm_lognormal_data_pass"
STUDENTT = "bsc_glm_studentt_data_pass"


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    nu = arg("--df", 4.0, float)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_studentt_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    W = 0.1 * torch.randn((S, D), generator=g, device=dev)
    logk = torch.linspace(-1.0, 1.0, S, device=dev)          # the eight tau of both scalar sides
    sets = []
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        loc = X @ torch.randn(D, generator=g, device=dev) + o
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        noise = 0.7 * torch.randn(N, generator=g, device=dev)
        # LogNormal(l, 0.7) durations; 30 % of the rows cut at a uniform fraction and flagged by the sign
        y = torch.exp(loc + noise).clamp_min(1e-30)
        cens = torch.rand(N, generator=g, device=dev) < 0.3
        cut = 0.1 + 0.9 * torch.rand(N, generator=g, device=dev)
        # the real-valued response: the same noise, a tenth of the rows with it times 20
        gross = torch.rand(N, generator=g, device=dev) < 0.1
        sets.append(dict(X=X, o=o, v=v, y=y, ys=torch.where(cens, -(y * cut).clamp_min(1e-30), y),
                         yr=loc + torch.where(gross, 20.0 * noise, noise)))
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
            if which == STUDENTT:
                ctx.call(STUDENTT, d["X"], D, d["yr"], d["o"], d["v"], N, D, W, logk, S, nu, ell, G, T)
            elif which == LOGNORMAL:
                ctx.call(LOGNORMAL, d["X"], D, d["ys"], d["o"], d["v"], N, D, W, logk, S, ell, G, T)
            else:
                ctx.call("bsc_glm_data_pass_obs", 1, d["X"], D, d["y"], d["o"], d["v"], N, D, W, S, ell, G)
        return one

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
                 "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                 "GBps": round(4.0 * N * (D + 3) / med[name] / 1e3, 1)})
        return med

    med = compare({name: pass_calls(name) for name in (POISSON, LOGNORMAL, STUDENTT)}, "pass")
    pass_ratio = {"studentt_over_poisson": round(med[STUDENTT] / med[POISSON], 4),
                  "studentt_over_lognormal": round(med[STUDENTT] / med[LOGNORMAL], 4),
                  "lognormal_over_poisson": round(med[LOGNORMAL] / med[POISSON], 4)}

    d0 = sets[0]
    kw = dict(n_samples=S, seed=3, lr=1e-3, ctx=ctx, offset=d0["o"], weights=d0["v"])
    models = {"GLMReparamSVI(poisson).step": (GLMReparamSVI(d0["X"], d0["y"], link="poisson", **kw), "y"),
              "LogNormalReparamSVI.step": (LogNormalReparamSVI(d0["X"], d0["ys"].abs(), d0["ys"] > 0, **kw), "ys"),
              "StudentTReparamSVI.step": (StudentTReparamSVI(d0["X"], d0["yr"], df=nu, **kw), "yr")}
    med = compare({name: update_calls(m, key) for name, (m, key) in models.items()}, "update")
    update_ratio = {"studentt_over_poisson": round(med["StudentTReparamSVI.step"] /
                                                   med["GLMReparamSVI(poisson).step"], 4),
                    "studentt_over_lognormal": round(med["StudentTReparamSVI.step"] /
                                                     med["LogNormalReparamSVI.step"], 4)}
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "df": nu, "pass": pass_ratio, "update": update_ratio, "byte_ratio": 1.0})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_studentt.py: us per call, median of %d alternating blocks of %d calls, %d rotating "
                "copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
