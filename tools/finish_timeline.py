"""Where does blr_fused_update_kernel spend its time, stage by stage?  Options blr_stamps + blr_finish_stamps: every
update of BLRReparamSVI leaves the pass's start / end stamps and, per finish workgroup, one s_memrealtime stamp per
stage (include/bayesic_hip.h, bsc_blr_read_stamps).  Printed, in us after the LAST pass workgroup's end: the stages of
the column workgroups (median and latest over the 32) and of the scalar workgroup, median over the updates, behind a
1M-row pass and behind a 125k-row pass.

    python tools/finish_timeline.py [updates] [rows ...]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from bayesic_amd.device import Context
from bayesic_amd.svi.blr import BLRReparamSVI

STAGES = ["wave start", "small operands landed", "slab summed", "after the workgroup barrier", "terms handed over (scalar)",
          "sums done (scalar)", "Adam done", "stores issued", "end"]


def timeline(ctx, B, updates, D=256, S=8):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(11)
    X = torch.randn((B, D), generator=g, device=dev)
    y = torch.randn(B, generator=g, device=dev)
    model = BLRReparamSVI(X, y, n_total=10 * B, n_samples=S, seed=1234, lr=0.01, ctx=ctx)
    n_fin = (D + 7) // 8 + 1
    rel, spans = [], []
    for i in range(updates + 5):
        model.step()
        st = ctx.read_stamps()
        if i < 5:
            continue
        n_pass = len(st) - 2 * n_fin
        assert n_pass > 0, "no pass stamps: %d rows" % len(st)
        pass_end = st[:n_pass, 1].max()
        fin = st[n_pass:].reshape(n_fin, 16)[:, :9].astype(np.int64)
        rel.append((fin - np.int64(pass_end)) / 100.0)
        spans.append((fin[:, 8].max() - fin[:, 0].min()) / 100.0)
    R = np.median(np.array(rel), 0)          # [workgroup, stage]
    col, sc = R[:-1], R[-1]
    print("rows %d: %d updates; finish span (first wave start .. last end) median %.2f us, min %.2f, max %.2f"
          % (B, updates, np.median(spans), min(spans), max(spans)))
    print("  %-30s %10s %10s %10s" % ("stage (us after the pass ends)", "col median", "col latest", "scalar"))
    for k, name in enumerate(STAGES):
        print("  %-30s %10.2f %10.2f %10.2f" % (name, np.median(col[:, k]), col[:, k].max(), sc[k]))
    print("  scalar workgroup, stage by stage (us): " + " ".join("%.2f" % v for v in np.diff(sc)))
    print("  column workgroups, stage by stage, median (us): " + " ".join("%.2f" % v for v in np.median(np.diff(col, axis=1), 0)))


def main():
    updates = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    rows = [int(v) for v in sys.argv[2:]] or [1_000_000, 125_000]
    ctx = Context(0, options=dict(blr_stamps=1, blr_finish_stamps=1))
    for B in rows:
        timeline(ctx, B, updates)


if __name__ == "__main__":
    main()
