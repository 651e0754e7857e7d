"""The grouped predictive pass against the pass it extends, in one process at BASELINE config 5's shape (1M x 256,
J = 1000; oracle.svi.make_cfg5's recipe, generated here), y and the offset set, every output requested:

    (a) bsc_predict_pass_offset         l = x . w + o                  (csrc/bsc_predict_offset.hip)
    (b) bsc_predict_pass_groups         l = x . w + b[g] + o           (csrc/bsc_predict_group.hip)

at S = 8 and S = 64 draws.  The algorithmic bytes of (b) over (a), per row: 4 for the id on 4 D + 12 = 1036 read and 12
written, x 1.004; the intercept table (4 (J + 1) ldb bytes: 64 KB at S = 8, 256 KB at S = 64) stays in the L2 / MALL.

Method (tools/bench_glm_group.py's): every case runs over ROTATE copies of the operands in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache; the second copy is the first with its rows rotated), is warmed
for at least 60 ms of back-to-back calls, and is then timed launch to launch in BLOCKS blocks of REPS calls between two
events.  (a) and (b) alternate block by block, so drift of the clocks or of a shared machine falls on both.  A line
reports the median block and the min-max spread.  Results go to stdout and to profiles/predict_group_bench.txt (--out).

    python tools/bench_predict_group.py [--rows N] [--groups J] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from oracle import svi  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
LOGISTIC = 1      # include/bayesic_hip.h: BSC_PREDICT_LOGISTIC


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D, J = arg("--rows", 1_000_000), 256, arg("--groups", 1000)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "predict_group_bench.txt"), str)
    ctx = Context(0)
    X, y, g, _, _ = svi.make_cfg5(N, D, J)
    g[::97] = -1                                     # some rows of a group that was not seen in training
    sets = [dict(X=ctx.to_device(X), y=ctx.to_device(y), g=ctx.to_device(g))]
    del X
    for k in range(1, ROTATE):
        sets.append({name: torch.roll(t, 4099 * k, 0).contiguous() for name, t in sets[0].items()})
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    for d in sets:
        d["o"] = 0.1 * torch.randn(N, generator=gen, device=ctx.device)
        ctx.call("bsc_group_ids_check", d["g"], N, J, 1)
    mean, var, lpd = ctx.zeros(N), ctx.zeros(N), ctx.zeros(N)
    lpd_sum = ctx.zeros(1, torch.float64)
    ctx.reserve(1 << 16)                             # lpd_sum's block partials
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % ROTATE]

    e0, e1 = ctx.event(), ctx.event()

    def block(fn, reps):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        return e0.elapsed_ms(e1)

    def measure(fns):
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
            say({"case": "%s %dx%d J=%d" % (name, N, D, J), "us": round(med[name], 2), "us_min": round(t[0], 2),
                 "us_max": round(t[-1], 2)})
        return med

    for S in (8, 64):
        ldb = 16 * ((S + 15) // 16)
        W = 0.1 * torch.randn((S, D), generator=gen, device=ctx.device)
        Bt = 0.5 * torch.randn((J + 1, ldb), generator=gen, device=ctx.device)

        def plain():
            d = nxt()
            ctx.call("bsc_predict_pass_offset", LOGISTIC, d["X"], D, d["y"], d["o"], N, D, W, None, S, mean, var, lpd,
                     lpd_sum)

        def grouped():
            d = nxt()
            ctx.call("bsc_predict_pass_groups", LOGISTIC, d["X"], D, d["y"], d["o"], d["g"], N, D, J, W, Bt, ldb, S, mean,
                     var, lpd, lpd_sum)

        m = measure({"(a) bsc_predict_pass_offset logistic S=%d" % S: plain,
                     "(b) bsc_predict_pass_groups logistic S=%d" % S: grouped})
        ctx.sync()
        ta, tb = list(m.values())
        say({"rows": N, "D": D, "J": J, "S": S, "groups_over_offset": round(tb / ta, 4),
             "byte_ratio": round((4.0 * D + 28) / (4.0 * D + 24), 4),
             "offset_fraction_of_8_TBps": round((4.0 * D + 24) * N / (ta * 1e-6) / 8e12, 3)})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_predict_group.py: us per call, median of %d alternating blocks of %d calls, %d rotating "
                "copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
