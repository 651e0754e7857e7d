"""The fixed tail of a regression update -- the pass's epilogue and the fused finish -- may be rescheduled but not
change a bit: five seeded updates of BLRReparamSVI against arrays recorded from the commit before the tail was
reworked (tests/golden/blr_tail_*.npy, written by `python tests/test_blr_tail_gpu.py --record` with that commit's library), compared
with ==.  Shapes: several workgroups with a ragged last tile on the 16-row kernel; S < 8 (the draws >= S of the slab
stay zero); the 8-row kernel at D < 256 and at D not a multiple of 8.  (D must be a multiple of 4 for every pass of
this library, so the smallest such D stands in for an odd one.)  Both entry points: bsc_blr_pass_update and, with
`family=`, bsc_blr_pass_update_general.

The stage stamps of the finish (option blr_finish_stamps) are a measurement aid: with them on the results are the
same bits, and every workgroup's stages are in order."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

SHAPES = [(4099, 256, 8), (2000, 256, 3), (1031, 200, 8), (517, 12, 5)]
ENTRIES = ["default", "general"]
UPDATES = 5
# a member of the family that is NOT config 2: other coefficients reach the finish through the _general entry point
FAMILY = (-3.25, -7.5, 10.0, 0.5, 2.0)


def golden_path(shape, entry):
    return os.path.join(GOLDEN, "blr_tail_%dx%dx%d_%s.npy" % (shape + (entry,)))


def run_updates(ctx, shape, entry):
    """[lam | grad | elbo | W] after UPDATES updates, as one float64 vector (W is float32: exact in float64)."""
    from bayesic_amd.svi.blr import BLRReparamSVI
    from oracle import svi
    B, D, S = shape
    X, y, _ = svi.make_cfg2(B, D)
    model = BLRReparamSVI(X, y, n_total=10 * B, n_samples=S, seed=4321, lr=0.01, ctx=ctx,
                          family=FAMILY if entry == "general" else None)
    for _ in range(UPDATES):
        model.step()
    ctx.sync()
    return np.concatenate([model.lam.cpu().numpy().ravel(), model.grad.cpu().numpy().ravel(),
                           model.elbo.cpu().numpy().ravel(), model.W.cpu().numpy().astype(np.float64).ravel()])


def split(shape, v):
    _, D, S = shape
    n = 2 * D + 2
    return dict(lam=v[:n], grad=v[n:2 * n], elbo=v[2 * n:2 * n + 1], W=v[2 * n + 1:])


@pytest.fixture(scope="module")
def ctx():
    from bayesic_amd.device import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture
def stamped_ctx():
    # one per test: the pass's rows are those of the context's LAST stamped 16-row pass, whichever update made it
    from bayesic_amd.device import Context
    c = Context(0, options=dict(blr_stamps=1, blr_finish_stamps=1))
    yield c
    c.close()


def assert_same_bits(shape, got, want):
    assert got.shape == want.shape
    g, w = split(shape, got), split(shape, want)
    for name in ("lam", "grad", "elbo", "W"):
        same = g[name] == w[name]
        assert same.all(), "%s differs in %d of %d entries (first at %d: %r != %r)" % (
            name, int((~same).sum()), same.size, int(np.argmin(same)), g[name][np.argmin(same)], w[name][np.argmin(same)])


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_five_updates_equal_the_recorded_bits(ctx, shape, entry):
    want = np.load(golden_path(shape, entry))
    assert np.isfinite(want).all()
    assert_same_bits(shape, run_updates(ctx, shape, entry), want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4099, 256, 8), (1031, 200, 8)], ids=lambda s: "%dx%dx%d" % s)
def test_stamps_change_no_bit_and_are_in_order(ctx, stamped_ctx, shape):
    B, D, S = shape
    plain = run_updates(ctx, shape, "default")
    assert_same_bits(shape, run_updates(stamped_ctx, shape, "default"), plain)
    st = stamped_ctx.read_stamps()
    n_fin = (D + 7) // 8 + 1
    n_pass = len(st) - 2 * n_fin
    # the 16-row pass (D = 256) leaves a row per workgroup; the 8-row pass is not stamped
    assert n_pass > 0 if D == 256 else n_pass == 0
    assert (st[:n_pass, 1] >= st[:n_pass, 0]).all() and (st[:n_pass, 0] > 0).all()
    fin = st[n_pass:].reshape(n_fin, 16)[:, :9].astype(np.int64)
    assert (fin[:, 0] > 0).all(), "a finish workgroup left no stamps"
    assert (np.diff(fin, axis=1) >= 0).all(), "stage stamps out of order:\n%s" % (fin - fin[:, :1])
    assert (fin[:, 8] > fin[:, 0]).all()
    if n_pass:
        # the finish is launched behind the pass on one stream
        assert fin[:, 0].min() >= st[:n_pass, 1].max()
    assert ctx.read_stamps().shape[0] == 0      # default off: nothing was stamped


def record(out_dir):
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from bayesic_amd.device import Context
    c = Context(0)
    for shape in SHAPES:
        for entry in ENTRIES:
            v = run_updates(c, shape, entry)
            assert np.isfinite(v).all(), (shape, entry)
            np.save(os.path.join(out_dir, os.path.basename(golden_path(shape, entry))), v)
            print("recorded", os.path.basename(golden_path(shape, entry)), v.shape, "elbo %.6f" % split(shape, v)["elbo"][0])
    c.close()


if __name__ == "__main__":
    if "--record" in sys.argv:      # --record [directory]
        at = sys.argv.index("--record") + 1
        record(sys.argv[at] if at < len(sys.argv) else GOLDEN)
