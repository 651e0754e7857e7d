"""The softmax-regression pass next to the logistic pass it was modelled on, in one process at 1M x 256 (rows:
--rows).  Each case is warmed for at least 60 ms of back-to-back calls and then timed in BLOCKS blocks of REPS calls
between two events; a line reports the median block and the min-max spread (tools/bench_glm.py's method):

  (a) bsc_glm_data_pass, logistic, S = 8                 (the yardstick: ONE launch reading the same bytes)
  (b) bsc_softmax_data_pass, S = 8, K = 2, 4, 10         (ceil(8 / floor(16 / K)) = 1, 2, 8 launches, each with its
                                                          slab reduction); per update and per launch
  (c) bsc_softmax_predict_pass, S = 64, K = 10           (one read of X; 64 draw groups inside the kernel)

Per launch: achieved TB/s on the algorithmic bytes 4 D + 8 per row (X, y and nothing else of size B) and TF on the
4 D flop per row and (draw, class) column that is occupied.  The figure of merit is (b) per launch over (a).

    python tools/bench_softmax.py [--rows N]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

BLOCKS, REPS = 7, 10


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(ctx, fn, reps=REPS, warm_ms=60.0):
    """us per call: (median, min, max) over BLOCKS blocks of `reps` calls."""
    e0, e1 = ctx.event(), ctx.event()
    elapsed = 0.0
    while elapsed < warm_ms:
        e0.record()
        fn()
        fn()
        e1.record()
        elapsed += e0.elapsed_ms(e1)
    blocks = []
    for _ in range(BLOCKS):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        blocks.append(e0.elapsed_ms(e1) / reps * 1e3)
    blocks.sort()
    return blocks[len(blocks) // 2], blocks[0], blocks[-1]


def main():
    N, D, S = arg("--rows", 1_000_000), 256, 8
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, D), generator=g, device=dev) / 16.0                 # logits of unit scale for unit-scale draws
    y_bern = (torch.rand(N, generator=g, device=dev) < 0.5).to(torch.float32)
    W1 = 0.1 * torch.randn((S, D), generator=g, device=dev)
    ell, G1 = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    row_bytes = 4.0 * D + 8.0

    def line(label, t, launches, cols):
        med, lo, hi = t
        per = med / launches
        out = {"case": label, "us": round(med, 1), "us_min": round(lo, 1), "us_max": round(hi, 1),
               "launches": launches, "us_per_launch": round(per, 1),
               "TBps_per_launch": round(N * row_bytes / per / 1e6, 2),
               "TF": round(4.0 * D * N * cols / med / 1e6, 1)}
        print(json.dumps(out), flush=True)
        return out

    t_a = timed(ctx, lambda: ctx.call("bsc_glm_data_pass", 0, X, D, y_bern, N, D, W1, S, ell, G1))
    a = line("(a) bsc_glm_data_pass logistic %dx%d S=%d" % (N, D, S), t_a, 1, S)
    ratios = {}
    for K in (2, 4, 10):
        y = torch.randint(0, K, (N,), generator=g, device=dev, dtype=torch.int32)
        W = 0.1 * torch.randn((S, K, D), generator=g, device=dev)
        G = ctx.zeros((S, K, D), torch.float64)
        per = 16 // K
        launches = (S + per - 1) // per
        t = timed(ctx, lambda: ctx.call("bsc_softmax_data_pass", X, D, y, N, D, K, W, S, ell, G))
        b = line("(b) bsc_softmax_data_pass K=%d S=%d" % (K, S), t, launches, S * K)
        ratios["K=%d" % K] = round(b["us_per_launch"] / a["us_per_launch"], 3)
    K, Sp = 10, 64
    y = torch.randint(0, K, (N,), generator=g, device=dev, dtype=torch.int32)
    W = 0.1 * torch.randn((Sp, K, D), generator=g, device=dev)
    prob, lpd = ctx.zeros((N, K)), ctx.zeros(N)
    lpd_sum = ctx.zeros(1, torch.float64)
    t = timed(ctx, lambda: ctx.call("bsc_softmax_predict_pass", X, D, y, N, D, K, W, Sp, prob, lpd, lpd_sum), reps=3)
    med = t[0]
    print(json.dumps({"case": "(c) bsc_softmax_predict_pass K=%d S=%d" % (K, Sp), "us": round(med, 1),
                      "us_min": round(t[1], 1), "us_max": round(t[2], 1),
                      "TBps": round(N * (row_bytes + 4.0 * K + 4.0) / med / 1e6, 2),
                      "TF": round(2.0 * D * N * Sp * K / med / 1e6, 1)}), flush=True)
    ctx.sync()
    print(json.dumps({"rows": N, "D": D, "softmax_per_launch_over_logistic_pass": ratios,
                      "spread_of_a": round((t_a[2] - t_a[0 + 1]) / t_a[0], 3)}), flush=True)


if __name__ == "__main__":
    main()
