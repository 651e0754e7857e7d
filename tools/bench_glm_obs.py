"""bsc_glm_data_pass against bsc_glm_data_pass_obs with offset AND weights set, in one process at 1M x 256, S = 8
(rows: --rows), both links.  The algorithmic byte ratio is (4 D + 12) / (4 D + 4) = 1036 / 1028 per row read: +0.8 %.

Method: every case runs over ROTATE copies of (X, y, o, v) in turn (1 GiB of X apiece: no call finds its operands in
the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then timed launch to launch in
BLOCKS blocks of REPS calls between two events.  The two entry points alternate block by block, so drift of the clocks
or of a shared machine falls on both.  A line reports the median block and the min-max spread; the last line is the
ratio of the medians per link.  Results go to stdout and to profiles/glm_obs_bench.txt (--out).

    python tools/bench_glm_obs.py [--rows N] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_obs_bench.txt"), str)
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    W = 0.1 * torch.randn((S, D), generator=g, device=dev)
    sets = []
    for _ in range(ROTATE):
        X = torch.randn((N, D), generator=g, device=dev) / 16.0
        o = 0.5 * torch.randn(N, generator=g, device=dev)
        logits = X @ torch.randn(D, generator=g, device=dev) + o
        v = 3.0 * torch.rand(N, generator=g, device=dev)
        v[::5] = 0.0
        sets.append(dict(X=X, o=o, v=v, logistic=(torch.rand(N, generator=g, device=dev) < torch.sigmoid(logits))
                         .to(torch.float32), poisson=torch.poisson(torch.exp(logits), generator=g)))
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    def calls(code, link, obs):
        turn = [0]

        def one():
            d = sets[turn[0] % ROTATE]
            turn[0] += 1
            if obs:
                ctx.call("bsc_glm_data_pass_obs", code, d["X"], D, d[link], d["o"], d["v"], N, D, W, S, ell, G)
            else:
                ctx.call("bsc_glm_data_pass", code, d["X"], D, d[link], N, D, W, S, ell, G)
        return one

    e0, e1 = ctx.event(), ctx.event()

    def block(fn, reps):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        return e0.elapsed_ms(e1)

    ratios = {}
    for code, link in ((0, "logistic"), (1, "poisson")):
        fns = {"bsc_glm_data_pass": calls(code, link, False), "bsc_glm_data_pass_obs": calls(code, link, True)}
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
            bytes_per_pass = 4.0 * N * (D + (3 if name.endswith("_obs") else 1))
            say({"case": "%s %s %dx%d S=%d" % (name, link, N, D, S), "us": round(med[name], 2),
                 "us_min": round(t[0], 2), "us_max": round(t[-1], 2),
                 "GBps": round(bytes_per_pass / med[name] / 1e3, 1)})
        ratios[link] = round(med["bsc_glm_data_pass_obs"] / med["bsc_glm_data_pass"], 4)
    ctx.sync()
    say({"rows": N, "D": D, "S": S, "obs_over_plain": ratios, "byte_ratio": round((4.0 * D + 12) / (4.0 * D + 4), 4)})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_obs.py: us per call, median of %d alternating blocks of %d calls, %d rotating copies "
                "of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
