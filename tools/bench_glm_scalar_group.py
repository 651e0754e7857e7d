"""The grouped pass of the families with a learned scalar against what it extends, in one process at 1M x 256,
J = 1000, S = 8, offset and weights set (simulated grouped data, generated here on the device).  Per family
(negative binomial, Gamma, Weibull):

    (a) bsc_glm_<family>_data_pass          the family's pass without groups
    (b) bsc_glm_scalar_data_pass_groups     the same link with the group ids, the gathered intercepts and the group sums
    (p) bsc_glm_data_pass_groups (Poisson)  the grouped pass without a learned scalar, on counts of the same rows
    (c) Hier<Family>ReparamSVI.step()       one whole update: (b), then bsc_glm_scalar_hier_update

The algorithmic bytes of (b) over (a), per row, are the grouped Poisson pass's: 4 for the id, 32 written and 32 re-read
for the residuals, 4 for the plan's permutation, on 4 D + 12 = 1036: x 1.07.

Method (tools/bench_glm_group.py's): every case runs over ROTATE copies of the operands in turn (1 GiB of X apiece: no
call finds its operands in the 256 MiB Infinity Cache), is warmed for at least 60 ms of back-to-back calls, and is then
timed launch to launch in BLOCKS blocks of REPS calls between two events; (a), (b) and (p) alternate block by block, so
drift of the clocks or of a shared machine falls on all of them.  A line reports the median block and the min-max
spread.  Results go to stdout and to profiles/glm_scalar_group_bench.txt (--out).

    python tools/bench_glm_scalar_group.py [--rows N] [--groups J] [--out FILE]
"""
import ctypes
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

BLOCKS, REPS, ROTATE = 9, 20, 2
FAMILIES = {"negbin": (0, "bsc_glm_nb_data_pass"), "gamma": (1, "bsc_glm_gamma_data_pass"),
            "weibull": (2, "bsc_glm_weibull_data_pass")}


def arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def responses(l, gen):
    """Counts, positive values and signed durations at the log mean (log scale) l, on l's device."""
    mu = torch.exp(l)
    e = -torch.log(torch.rand(l.shape, generator=gen, device=l.device).clamp_min(1e-12))      # Exp(1)
    t = (mu * e.pow(1.0 / 1.5)).clamp_min(1e-20)
    cens = torch.rand(l.shape, generator=gen, device=l.device) < 0.3
    return dict(negbin=torch.poisson(mu, generator=gen), gamma=(mu * e).clamp_min(1e-20),
                weibull=torch.where(cens, -0.5 * t, t))


def main():
    from bayesic_amd import svi
    N, D, S, J = arg("--rows", 1_000_000), 256, 8, arg("--groups", 1000)
    out_path = arg("--out", os.path.join(ROOT, "profiles", "glm_scalar_group_bench.txt"), str)
    ctx = Context(0)
    gen = torch.Generator(device=ctx.device).manual_seed(0)
    X = torch.randn((N, D), generator=gen, device=ctx.device) / math.sqrt(D)
    g = torch.randint(J, (N,), generator=gen, device=ctx.device, dtype=torch.int32)
    l = X @ (0.5 * torch.randn(D, generator=gen, device=ctx.device)) + \
        0.5 * torch.randn(J, generator=gen, device=ctx.device)[g.long()]
    first = dict(X=X, g=g, o=0.1 * torch.randn(N, generator=gen, device=ctx.device),
                 v=torch.rand(N, generator=gen, device=ctx.device) + 0.5, **responses(l, gen))
    del X, l
    sets = [first] + [{name: torch.roll(t, 4099 * k, 0).contiguous() for name, t in first.items()}
                      for k in range(1, ROTATE)]
    for d in sets:
        n = ctx.lib.bsc_glm_group_plan_size(N, J)
        d["plan"] = torch.zeros(n, dtype=torch.int32, device=ctx.device)
        ctx.call("bsc_glm_group_plan", d["g"], N, J, d["plan"], ctypes.byref(ctypes.c_int32(0)))
    ctx.reserve(int(ctx.lib.bsc_glm_scalar_group_workspace_bytes(ctx.handle, N, J)))
    W = 0.1 * torch.randn((S, D), generator=gen, device=ctx.device)
    Bz = 0.5 * torch.randn(J * 8, generator=gen, device=ctx.device)
    logtau = 0.3 * torch.randn(S, generator=gen, device=ctx.device)
    f64 = torch.float64
    ell, G, H, T = ctx.zeros(S, f64), ctx.zeros((S, D), f64), ctx.zeros((S, J), f64), ctx.zeros(S, f64)
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
            say({"case": "%s %dx%d J=%d S=%d" % (name, N, D, J, S), "us": round(med[name], 2),
                 "us_min": round(t[0], 2), "us_max": round(t[-1], 2)})
        return med

    def poisson_groups():
        d = nxt()
        ctx.call("bsc_glm_data_pass_groups", 1, d["X"], D, d["negbin"], d["o"], d["v"], d["g"], d["plan"], N, D, J, W, Bz,
                 S, ell, G, H)

    classes = {"negbin": svi.HierNegBinReparamSVI, "gamma": svi.HierGammaReparamSVI,
               "weibull": svi.HierWeibullReparamSVI}
    for fam, (code, plain_name) in FAMILIES.items():
        def plain():
            d = nxt()
            ctx.call(plain_name, d["X"], D, d[fam], d["o"], d["v"], N, D, W, logtau, S, ell, G, T)

        def grouped():
            d = nxt()
            ctx.call("bsc_glm_scalar_data_pass_groups", code, d["X"], D, d[fam], d["o"], d["v"], d["g"], d["plan"], N, D,
                     J, W, Bz, logtau, S, ell, G, H, T)

        d0 = sets[0]
        y0 = d0[fam].abs() if fam == "weibull" else d0[fam]
        kw = dict(event=d0[fam] > 0) if fam == "weibull" else {}
        model = classes[fam](d0["X"], y0, d0["g"], J, n_samples=S, seed=5, lr=1e-3, offset=d0["o"], weights=d0["v"],
                             ctx=ctx, **kw)
        plans = [model.build_plan(d["g"], N) for d in sets]

        def update():
            k = turn[0] = turn[0] + 1
            d = sets[k % ROTATE]
            # the rotation's own plan, built above, and raw pointers (taken as they are): no synchronisation in the loop
            model.set_batch(d["X"].data_ptr(), d[fam].data_ptr(), rows=N, offset=d["o"].data_ptr(),
                            weights=d["v"].data_ptr(), groups=d["g"].data_ptr(), plan=plans[k % ROTATE])
            model.step()

        m = measure({"(a) %s" % plain_name: plain, "(b) bsc_glm_scalar_data_pass_groups %s" % fam: grouped,
                     "(p) bsc_glm_data_pass_groups poisson": poisson_groups})
        c = measure({"(c) Hier %s step" % fam: update})
        ctx.sync()
        ta, tb, tp = list(m.values())
        say({"family": fam, "rows": N, "D": D, "J": J, "groups_over_ungrouped": round(tb / ta, 4),
             "over_poisson_groups": round(tb / tp, 4), "byte_ratio": round((4.0 * D + 12 + 72) / (4.0 * D + 12), 4),
             "update_over_pass": round(list(c.values())[0] / tb, 4)})
        del model
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("# tools/bench_glm_scalar_group.py: us per call, median of %d alternating blocks of %d calls, %d rotating "
                "copies of the operands\n" % (BLOCKS, REPS, ROTATE))
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
