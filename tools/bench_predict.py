"""The predictive pass against the read probe and the GLM training pass, in one process on one resident 1M x 256
buffer (rows: --rows).  Cases are timed in alternated repeats (ROUNDS rounds over all cases, each case a block of REPS
back-to-back calls between two events, after a common warm-up); a line reports the median block and the min-max spread:

  (a) bsc_hbm_read_probe on the same buffer                         (the yardstick: (c) is quoted as a fraction of it)
  (b) bsc_glm_data_pass, logistic, S = 8                            (the training pass on the same bytes)
  (c) bsc_predict_pass, each family at S = 8 and S = 64, all four outputs requested

Conditions: (c) at S = 8 is not slower than (b); (c) at S = 64 is far below 8 x (c) at S = 8 (X is read once).

    python tools/bench_predict.py [--rows N]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bayesic_amd.device import Context  # noqa: E402

ROUNDS, REPS = 7, 20


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    N, D = arg("--rows", 1_000_000), 256
    ctx = Context(0)
    dev = ctx.device
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, D), generator=g, device=dev) / 16.0
    logits = X @ torch.randn(D, generator=g, device=dev)
    y = {0: logits + 0.5 * torch.randn(N, generator=g, device=dev),
         1: (torch.rand(N, generator=g, device=dev) < torch.sigmoid(logits)).to(torch.float32),
         2: torch.poisson(torch.exp(logits), generator=g)}
    W = 0.1 * torch.randn((64, D), generator=g, device=dev)
    logvar = torch.rand(64, generator=g, device=dev) - 1.0
    ell, G = ctx.zeros(8, torch.float64), ctx.zeros((8, D), torch.float64)
    mean, var, lpd = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
    lpd_sum = ctx.zeros(1, torch.float64)
    bytes_x = 4.0 * N * (D + 1)

    cases = [("(b) bsc_glm_data_pass logistic S=8",
              lambda: ctx.call("bsc_glm_data_pass", 0, X, D, y[1], N, D, W, 8, ell, G))]
    for S in (8, 64):
        for code, name in ((0, "gaussian"), (1, "logistic"), (2, "poisson")):
            cases.append(("(c) bsc_predict_pass %s S=%d" % (name, S),
                          lambda code=code, S=S: ctx.call("bsc_predict_pass", code, X, D, y[code], N, D, W, logvar, S,
                                                          mean, var, lpd, lpd_sum)))
    e0, e1 = ctx.event(), ctx.event()
    elapsed = 0.0
    while elapsed < 100.0:                    # common warm-up
        e0.record()
        for _, fn in cases:
            fn()
        e1.record()
        elapsed += e0.elapsed_ms(e1)
    blocks = {label: [] for label, _ in cases}
    probe = []
    for _ in range(ROUNDS):
        probe.append(ctx.read_probe(X, reps=10))
        for label, fn in cases:
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            blocks[label].append(e0.elapsed_ms(e1) / REPS * 1e3)
    probe.sort()
    probe_gbs = probe[len(probe) // 2]
    probe_us = 4.0 * N * D / probe_gbs / 1e3
    print(json.dumps({"case": "(a) bsc_hbm_read_probe %dx%d" % (N, D), "GBps": round(probe_gbs, 1),
                      "GBps_min": round(probe[0], 1), "GBps_max": round(probe[-1], 1), "us": round(probe_us, 2)}), flush=True)
    med = {}
    for label, _ in cases:
        b = sorted(blocks[label])
        med[label] = b[len(b) // 2]
        print(json.dumps({"case": label, "us": round(med[label], 2), "us_min": round(b[0], 2), "us_max": round(b[-1], 2),
                          "GBps": round(bytes_x / med[label] / 1e3, 1),
                          "fraction_of_probe": round(bytes_x / med[label] / 1e3 / probe_gbs, 3)}), flush=True)
    t_b = med[cases[0][0]]
    summary = {"rows": N, "D": D}
    ok = True
    for name in ("gaussian", "logistic", "poisson"):
        t8, t64 = med["(c) bsc_predict_pass %s S=8" % name], med["(c) bsc_predict_pass %s S=64" % name]
        summary[name] = {"s8_over_glm_pass": round(t8 / t_b, 3), "s64_over_s8": round(t64 / t8, 3)}
        ok = ok and t8 <= t_b and t64 < 4.0 * t8
    summary["conditions_hold"] = ok
    print(json.dumps(summary), flush=True)
    if not ok:
        sys.exit("the predictive pass missed a condition (S = 8 no slower than the GLM pass; S = 64 well under 8 x S = 8)")


if __name__ == "__main__":
    main()
