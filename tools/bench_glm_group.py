"""The grouped GLM pass and the random-intercept update against what they replace, in one process at BASELINE config 5's
shape (1M x 256, J = 1000; oracle.svi.make_cfg5's recipe, generated here):

    (a) bsc_glm_data_pass_obs           the pass without groups (offset and weight set: the grouped kernels are
                                        its bodies)
    (b) bsc_glm_data_pass_groups        the same pass with the group ids, the gathered intercepts and the group sums
    (c) HierGLMReparamSVI.step()        one pathwise update at S = 8: (b) without offset and weight, then
                                        bsc_glm_hier_update
    (d) LogRegBBVI.step()               one score-function update at S = 64 (svi/bbvi.py), the route config 5 had

The algorithmic bytes of (b) over (a), per row: 4 for the id, 32 written and 32 re-read for the residuals, 4 for the
plan's permutation, on 4 D + 12 = 1036: x 1.07.

Method: every case runs over ROTATE copies of the operands in turn (1 GiB of X apiece: no call finds its operands in
the 256 MiB Infinity Cache; the second copy is the first with its rows rotated), is warmed for at least 60 ms of
back-to-back calls, and is then timed launch to launch in BLOCKS blocks of REPS calls between two events ((d) has no
set_batch and stays on the first copy, whose 1 GiB does not survive in the cache between updates).  (a) and (b)
alternate block by block, and so do (c) and (d), so drift of the clocks or of a shared machine falls on both.  A line
reports the median block and the min-max spread.  Results go to stdout and to profiles/glm_group_bench.txt (--out).

    python tools/bench_glm_group.py [--rows N] [--groups J] [--out FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctypes  # noqa: E402

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402
from oracle import svi  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    from bayesic_amd.svi import HierGLMReparamSVI
    from bayesic_amd.svi.bbvi import LogRegBBVI
    N, D, S, J = arg("--rows", 1_000_000), 256, 8, arg("--groups", 1000)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_group_bench.txt"), str)
    ctx = Context(0)
    X, y, g, _, _ = svi.make_cfg5(N, D, J)
    sets = [dict(X=ctx.to_device(X), y=ctx.to_device(y), g=ctx.to_device(g))]
    del X
    for k in range(1, ROTATE):
        sets.append({name: torch.roll(t, 4099 * k, 0).contiguous() for name, t in sets[0].items()})
    for d in sets:
        d["o"], d["v"] = ctx.zeros(N), torch.ones(N, dtype=torch.float32, device=ctx.device)
        n = ctx.lib.bsc_glm_group_plan_size(N, J)
        d["plan"] = torch.zeros(n, dtype=torch.int32, device=ctx.device)
        ctx.call("bsc_glm_group_plan", d["g"], N, J, d["plan"], ctypes.byref(ctypes.c_int32(0)))
    ctx.reserve(int(ctx.lib.bsc_glm_group_workspace_bytes(ctx.handle, N, J)))
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    W = 0.1 * torch.randn((S, D), generator=gen, device=ctx.device)
    Bz = 0.5 * torch.randn(J * 8, generator=gen, device=ctx.device)
    f64 = torch.float64
    ell, G, H = ctx.zeros(S, f64), ctx.zeros((S, D), f64), ctx.zeros((S, J), f64)
    lines = []

    def say(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    turn = [0]

    def nxt():
        turn[0] += 1
        return sets[turn[0] % ROTATE]

    def plain():
        d = nxt()
        ctx.call("bsc_glm_data_pass_obs", 0, d["X"], D, d["y"], d["o"], d["v"], N, D, W, S, ell, G)

    def grouped():
        d = nxt()
        ctx.call("bsc_glm_data_pass_groups", 0, d["X"], D, d["y"], d["o"], d["v"], d["g"], d["plan"], N, D, J, W, Bz, S,
                 ell, G, H)

    d0 = sets[0]
    hier = HierGLMReparamSVI(d0["X"], d0["y"], d0["g"], J, n_samples=S, seed=5, lr=1e-3, ctx=ctx)
    bbvi = LogRegBBVI(d0["X"], d0["y"], d0["g"], J, n_total=float(N), n_samples=64, seed=5, lr=1e-3, ctx=ctx)
    plans = [(hier.plan, hier.n_segments)] + [hier._build_plan(d["g"], N) for d in sets[1:]]

    def hier_step():
        k = turn[0] = turn[0] + 1
        d = sets[k % ROTATE]
        # the rotation's own plan, built above: what set_batch(groups=) does, without its synchronisation in the loop
        hier.X, hier.y, hier._Xarg, hier._yarg = d["X"], d["y"], d["X"], d["y"]
        hier._set_groups(d["g"], plans[k % ROTATE])
        hier.step()

    def bbvi_step():
        bbvi.step()

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

    a = measure({"(a) bsc_glm_data_pass_obs logistic S=8": plain, "(b) bsc_glm_data_pass_groups logistic S=8": grouped})
    b = measure({"(c) HierGLMReparamSVI.step S=8": hier_step, "(d) LogRegBBVI.step S=64": bbvi_step})
    ctx.sync()
    ta, tb = list(a.values())
    tc, td = list(b.values())
    say({"rows": N, "D": D, "J": J, "groups_over_obs": round(tb / ta, 4),
         "byte_ratio": round((4.0 * D + 12 + 72) / (4.0 * D + 12), 4), "bbvi_over_hier": round(td / tc, 3)})
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_group.py: us per call, median of %d alternating blocks of %d calls, %d rotating copies "
                "of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
