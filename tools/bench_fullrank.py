"""Milliseconds per update of config 2 (1M x 256, S = 8) with the full-covariance guide beside the mean-field one,
timed the way tools/bench_configs.py times its rows (device events around a steady train of updates), plus the two
finish kernels alone on the same inputs.  The two drivers are timed twice, alternating, to show the spread.

    python tools/bench_fullrank.py [--quick]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch

from bayesic_amd.device import Context
from bayesic_amd.svi.blr import BLRReparamSVI
from bench_configs import LAST_DISTRIBUTION, timed


def main():
    quick = "--quick" in sys.argv
    N, D, S = (250_000 if quick else 1_000_000), 256, 8
    reps = 20 if quick else 100
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, D), generator=g, device=dev)
    y = X @ (torch.randn(D, generator=g, device=dev) / 16.0) + 0.5 * torch.randn(N, generator=g, device=dev)
    models = {cov: BLRReparamSVI(X, y, n_samples=S, seed=1234, lr=0.01, ctx=ctx, covariance=cov)
              for cov in ("diag", "full")}

    def emit(rec):
        rec.update(call_median_us=LAST_DISTRIBUTION.get("median_us"), call_min_us=LAST_DISTRIBUTION.get("min_us"))
        print(json.dumps(rec), flush=True)

    for rnd in range(2):
        for cov, m in models.items():
            wall, kern = timed(ctx, m.step, reps, warm=10)
            emit(dict(config="cfg2 BLRReparamSVI %dx%d S=%d covariance=%s" % (N, D, S, cov), round=rnd,
                      ms_per_step=wall * 1e3, pass_kernel_us=kern * 1e6, n_lam=int(m.lam.numel())))
    ctx.sync()
    # the two finishes alone, on the state the drivers left (stats of their last pass)
    for cov, m in models.items():
        c, n = m.cur, 1 - m.cur
        name = "bsc_blr_fullrank_update" if cov == "full" else "bsc_blr_fused_update_general"
        fam = m._nig_family()
        call = lambda m=m, name=name, fam=fam, c=c, n=n: ctx.call(
            name, m.stats, m._lam[c], m._lam[n], m.m1, m.m2, m._eps[0], m._W[c], m._xi[c], D, S, *fam, 1, 0.0,
            0.9, 0.999, 1e-8, m.seed, 1, m._eps[1], 1, m._W[n], m._xi[n], m.elbo, m.grad)
        wall, _ = timed(ctx, call, reps, warm=10)
        ctx.profile(True)                   # the finish kernel's own slot (event pair around each launch)
        for _ in range(reps):
            call()
        ms, cnt = ctx.profile_read(2)
        ctx.profile(0)
        emit(dict(config="finish alone: %s D=%d S=%d" % (name, D, S), us_per_call=wall * 1e6,
                  finish_kernel_us=ms / max(cnt, 1) * 1e3))


if __name__ == "__main__":
    main()
