"""The mixture's predictive pass at config 3's shape (10M x 16 rows, K = 64): bsc_mog_predict_pass with lpd and label,
with R as well, and with lpd_sum alone, beside bsc_mog_estep on the same X -- one process, alternating blocks, medians
and spreads over the blocks.
    python tools/bench_mog_predict.py [--rows N] [--blocks B] [--calls C] [--out FILE]

The two limits the measured time is held against:
 * HBM: 64 B in and 8 B out per row without R (4 K more with it), at the 6.29 TB/s a copy reaches on this part;
 * VALU: per (row, component, column) the compiled loop (mog_predict_kernel<true, false>, gfx950 ISA) issues 12 vector
   instructions -- v_subrev, 4 v_mul, 2 v_add, v_cmp, v_cndmask, v_fmac and the two transcendental v_log, v_rcp -- at 4
   cycles each, 8 for a transcendental: 56 cycles for the 64 rows of a wave on one of the chip's 4 x CU SIMDs."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayesic_amd.device import Context     # noqa: E402

HBM_COPY_TBS = 6.29
VECTOR_PER_TERM, TRANS_PER_TERM = 12, 2
CYCLES_PER_TERM = 4 * (VECTOR_PER_TERM - TRANS_PER_TERM) + 8 * TRANS_PER_TERM


def fitted_eta(cen, n_k):
    """The eta a converged fit has on unit-spread clusters at `cen` with n_k rows each (prior 1, 0, 0.01, 1, 1)."""
    K, D = cen.shape
    kappa = np.full((K, D), 0.01 + n_k)
    a = np.full((K, D), 1.0 + 0.5 * n_k)
    b = 1.0 + 0.5 * n_k * np.ones((K, D))
    return np.concatenate([np.full(K, float(n_k)), (kappa * cen).ravel(), kappa.ravel(), (2 * a - 1).ravel(),
                           (2 * b + kappa * cen * cen).ravel()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, D, K = args.rows, 16, 64
    ctx = Context(0)
    info = ctx.info()
    g = torch.Generator(device=ctx.device).manual_seed(23)
    cen = torch.randn((K, D), generator=g, device=ctx.device) * 4
    X = cen[torch.randint(K, (N,), generator=g, device=ctx.device)] + torch.randn((N, D), generator=g, device=ctx.device)
    eta = ctx.to_device(fitted_eta(cen.double().cpu().numpy(), N / K), torch.float64)
    Pt, c = ctx.empty((K, 3 * D)), ctx.empty(K)
    ctx.call("bsc_mog_predictive_params", eta, K, D, Pt, c)
    Wmat, cw = ctx.empty((K, 2 * D)), ctx.empty(K)
    ctx.call("bsc_mog_expected_params", eta, K, D, Wmat, cw)
    lpd, label, R = ctx.empty(N), ctx.empty(N, torch.int32), ctx.empty((N, K))
    lpd_sum = ctx.zeros(1, torch.float64)
    stats, lse = ctx.zeros((K, 1 + 2 * D), torch.float64), ctx.zeros(1, torch.float64)
    runs = {
        "predict: lpd, label": lambda: ctx.call("bsc_mog_predict_pass", X, D, N, D, K, Pt, c, lpd, label, None, K, None),
        "predict: lpd, label, R": lambda: ctx.call("bsc_mog_predict_pass", X, D, N, D, K, Pt, c, lpd, label, R, K, None),
        "predict: lpd_sum only": lambda: ctx.call("bsc_mog_predict_pass", X, D, N, D, K, Pt, c, None, None, None, K,
                                                  lpd_sum),
        "bsc_mog_estep": lambda: ctx.call("bsc_mog_estep", X, D, N, D, K, Wmat, cw, stats, lse),
    }
    for run in runs.values():           # warm every shape the timed window uses
        for _ in range(3):
            run()
    ctx.sync()
    times = {name: [] for name in runs}
    for _ in range(args.blocks):        # alternating blocks
        for name, run in runs.items():
            e0, e1 = ctx.event(), ctx.event()
            e0.record()
            for _ in range(args.calls):
                run()
            e1.record()
            times[name].append(e0.elapsed_ms(e1) / args.calls)
    # what the pass computed, against float64 on a sample
    idx = torch.arange(0, N, max(N // 4096, 1), device=ctx.device)
    x = X[idx].double()
    P = Pt.double()
    t = (P[None, :, 2 * D:] * torch.log1p(P[None, :, D:2 * D] * (x[:, None, :] - P[None, :, :D]) ** 2)).sum(2)
    want = torch.logsumexp(c.double()[None] - t, 1)
    err = (lpd[idx].double() - want).abs().max().item()

    lines = ["bsc_mog_predict_pass at %d x %d, K = %d on %d CUs at %.2f GHz; %d blocks of %d calls, alternating"
             % (N, D, K, info["cu_count"], info["clock_khz"] * 1e-6, args.blocks, args.calls)]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append("%-24s median %8.1f us   min %8.1f   max %8.1f" % (name, med[name] * 1e3, min(ts) * 1e3, max(ts) * 1e3))
    base = med["predict: lpd, label"]
    hbm_ms = N * (4.0 * D + 8.0) / (HBM_COPY_TBS * 1e12) * 1e3
    valu_ms = (N / 64.0) * K * D * CYCLES_PER_TERM / (4.0 * info["cu_count"]) / (info["clock_khz"] * 1e3) * 1e3
    lines.append("ratio to bsc_mog_estep: %.2f (lpd, label), %.2f (with R), %.2f (lpd_sum only)"
                 % (base / med["bsc_mog_estep"], med["predict: lpd, label, R"] / med["bsc_mog_estep"],
                    med["predict: lpd_sum only"] / med["bsc_mog_estep"]))
    lines.append("limits without R: HBM %.0f us (72 B a row at %.2f TB/s), VALU %.0f us (%d vector instructions a term, %d of "
                 "them transcendental: %d cycles a wave-term at the reported clock); measured / HBM %.1f, measured / VALU %.2f"
                 % (hbm_ms * 1e3, HBM_COPY_TBS, valu_ms * 1e3, VECTOR_PER_TERM, TRANS_PER_TERM, CYCLES_PER_TERM,
                    base / hbm_ms, base / valu_ms))
    lines.append("the time is nearer to its %s limit" % ("VALU" if abs(base - valu_ms) < abs(base - hbm_ms) else "HBM"))
    lines.append("max |lpd - float64| over %d sampled rows: %.2e (lpd_sum / N = %.6f)" % (idx.numel(), err, lpd_sum.item() / N))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
