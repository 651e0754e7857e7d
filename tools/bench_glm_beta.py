"""bsc_glm_beta_data_pass against bsc_glm_data_pass_obs with the logistic link (its bytes-equal neighbour: the same
logit) and bsc_glm_nb_data_pass, offset AND weights set on all three, in one process at 1M x 256, S = 8 (rows: --rows);
then one BetaReparamSVI update against one NegBinReparamSVI update on the same rows.  The passes read the same bytes,
4 D + 12 per row (the eight tau are 32 bytes per launch): the byte ratio is 1.000, and what the ratio of the times shows
is the cost of the link -- per (row, draw) the logistic link is one exp, one log and a reciprocal; the negative binomial
adds ONE shifted product of up to eight factors with its log and reciprocal (none for a whole count up to 8 beyond the
product itself); the Beta link evaluates TWO such products, at m phi and (1 - m) phi, with two logs and two reciprocals
each, and the logs of y and 1 - y.  The expectation to confirm or refute: logistic <= negative binomial <= Beta.

Method (tools/bench_glm_nb.py's): every case runs over ROTATE copies of (X, y, o, v) in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then
timed launch to launch in BLOCKS blocks of REPS calls between two events.  The sides alternate block by block, so
drift of the clocks or of a shared machine falls on all of them.  A line reports the median block and the min-max
spread.  The logistic side reads a Bernoulli y of the same mean, the Beta side a Beta(5 m, 5 (1 - m)) response clipped
to [1e-6, 1 - 1e-6], the negative binomial counts of mean e^{l}.  Results go to stdout and to
profiles/glm_beta_bench.txt (--out).

    python tools/bench_glm_beta.py [--rows N] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from bayesic_amd.svi import BetaReparamSVI, NegBinReparamSVI  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
LOGISTIC, BETA, NEGBIN = "bsc_glm_data_pass_obs(logistic)", "bsc_glm_beta_data_pass", "bsc_glm_nb_data_pass"


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_beta_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    W = 0.1 * torch.randn((S, D), generator=g, device=dev)
    logtau = torch.linspace(-1.0, 3.0, S, device=dev)        # log precision / log dispersion of the eight draws
    sets = []
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        l = X @ torch.randn(D, generator=g, device=dev) + o
        m = torch.sigmoid(l)
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        y = torch.distributions.Beta(5.0 * m, 5.0 * (1.0 - m)).sample().clamp(1e-6, 1.0 - 1e-6)
        sets.append(dict(X=X, o=o, v=v, y=y, yb=torch.bernoulli(m, generator=g),
                         yc=torch.poisson(torch.exp(l), generator=g)))
        del l, m
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
            if which == BETA:
                ctx.call(BETA, d["X"], D, d["y"], d["o"], d["v"], N, D, W, logtau, S, ell, G, T)
            elif which == NEGBIN:
                ctx.call(NEGBIN, d["X"], D, d["yc"], d["o"], d["v"], N, D, W, logtau, S, ell, G, T)
            else:
                ctx.call("bsc_glm_data_pass_obs", 0, d["X"], D, d["yb"], d["o"], d["v"], N, D, W, S, ell, G)
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

    med = compare({name: pass_calls(name) for name in (LOGISTIC, BETA, NEGBIN)}, "pass")
    pass_ratio = round(med[BETA] / med[LOGISTIC], 4)
    nb_ratio = round(med[NEGBIN] / med[LOGISTIC], 4)
    beta_over_nb = round(med[BETA] / med[NEGBIN], 4)

    d0 = sets[0]
    kw = dict(n_samples=S, seed=3, lr=1e-3, ctx=ctx, offset=d0["o"], weights=d0["v"])
    models = {"NegBinReparamSVI.step": (NegBinReparamSVI(d0["X"], d0["yc"], **kw), "yc"),
              "BetaReparamSVI.step": (BetaReparamSVI(d0["X"], d0["y"], **kw), "y")}
    med = compare({name: update_calls(m, key) for name, (m, key) in models.items()}, "update")
    update_ratio = round(med["BetaReparamSVI.step"] / med["NegBinReparamSVI.step"], 4)
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "beta_over_logistic": {"pass": pass_ratio}, "nb_over_logistic": {"pass": nb_ratio},
         "beta_over_nb": {"pass": beta_over_nb, "update": update_ratio}, "byte_ratio": 1.0,
         "nb_between_logistic_and_beta": bool(1.0 <= nb_ratio <= pass_ratio)})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_beta.py: us per call, median of %d alternating blocks of %d calls, %d rotating "
                "copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
