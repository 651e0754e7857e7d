"""bsc_glm_ordinal_data_pass (K = 5) against bsc_glm_data_pass_obs with the logistic link, offset AND weights set on
both, in one process at 1M x 256, S = 8 (rows: --rows).  The passes read the same bytes per row, 4 D + 12 (the labels
are four bytes like the logistic side's float y; the draws are 8 x 260 floats per launch against 8 x 256): the byte ratio
is 1.000.  The ordinal link is two softplus / sigmoid pairs and seven select-adds per (row, draw) where the logistic one
is one pair, so the expectation to confirm or refute is that both passes are bound by HBM and take the same time.

Method (tools/bench_glm_weibull.py's): every case runs over ROTATE copies of (X, y, o, v) in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then
timed launch to launch in BLOCKS blocks of REPS calls between two events.  The sides alternate block by block, so
drift of the clocks or of a shared machine falls on both.  A line reports the median block and the min-max spread.
The labels are drawn from the model at cutpoints -1.5, -0.5, 0.5, 1.5; the logistic side reads [label >= 2] as its
response.  Results go to stdout and to profiles/glm_ordinal_bench.txt (--out).

    python tools/bench_glm_ordinal.py [--rows N] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
LOGISTIC, ORDINAL = "bsc_glm_data_pass_obs(logistic)", "bsc_glm_ordinal_data_pass"


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S, K = arg("--rows", 1_000_000), 256, 8, 5
    P = D + K - 1
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_ordinal_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    Z = torch.zeros((S, P), device=dev)
    Z[:, :D] = 0.1 * torch.randn((S, D), generator=g, device=dev)
    Z[:, D] = -1.5 + 0.1 * torch.randn(S, generator=g, device=dev)      # theta_0 = c_0; the log-gaps stay near 0
    Z[:, D + 1:] = 0.1 * torch.randn((S, K - 2), generator=g, device=dev)
    W = Z[:, :D].contiguous()
    cuts = torch.tensor([-1.5, -0.5, 0.5, 1.5], device=dev)
    sets = []
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        eta = X @ torch.randn(D, generator=g, device=dev) + o
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        u = torch.rand(N, generator=g, device=dev)
        y = (u[:, None] > torch.sigmoid(cuts[None, :] - eta[:, None])).sum(dim=1).to(torch.int32)
        sets.append(dict(X=X, o=o, v=v, y=y, yb=(y >= 2).to(torch.float32)))
    shares = [round(float(sum((d["y"] == k).float().mean().item() for d in sets) / ROTATE), 4) for k in range(K)]
    ell, G, Gw = ctx.zeros(S, torch.float64), ctx.zeros((S, P), torch.float64), ctx.zeros((S, D), torch.float64)
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    def pass_calls(which):
        turn = [0]

        def one():
            d = sets[turn[0] % ROTATE]
            turn[0] += 1
            if which == ORDINAL:
                ctx.call(ORDINAL, d["X"], D, d["y"], d["o"], d["v"], N, D, K, Z, P, S, ell, G)
            else:
                ctx.call("bsc_glm_data_pass_obs", 0, d["X"], D, d["yb"], d["o"], d["v"], N, D, W, S, ell, Gw)
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

    med = compare({name: pass_calls(name) for name in (LOGISTIC, ORDINAL)}, "pass")
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "K": K, "level_shares": shares,
         "pass": {"ordinal_over_logistic": round(med[ORDINAL] / med[LOGISTIC], 4)}, "byte_ratio": 1.0})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_ordinal.py: us per call, median of %d alternating blocks of %d calls, %d rotating "
                "copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
