"""bsc_logreg_bbvi_loglik where a resident wave runs MORE THAN TWO tiles: the cases that use the X ring's wrap into the
next tile, the y / id double buffers at parity 0, 1, 0 (, 1) and the descriptor of the tile after the last one
(csrc/bsc_bbvi.hip: logreg_loglik_dma_kernel, logreg_loglik_dma_bx_kernel, logreg_loglik_xreg_kernel).
tests/test_bbvi_gpu.py stops at N = 20 000, at most one tile per wave on 256 CUs, and only the split route sees
N = 70 001 (tests/test_mfma_split_gpu.py); at such N the bound 2e-5 * sum(|l| + 1) is wider than one whole lost row,
hence the exact accounting below.

Shapes come from the device.  `grid` restates the host arithmetic of bsc_logreg_bbvi_loglik: 16-row tiles,
n_waves = 8 * min(cu, ceil(n_tiles / 8)), n_iter = ceil(n_tiles / n_waves) rounded up to even; wave w takes tiles
w, w + n_waves, ...  N = k (8 cu 16) + 16 + 5 is k full sweeps, one full tile and a ragged one of five rows: k + 1 tiles
on the first two waves and k on the rest.  k = 2 (65 557 rows at 256 CUs): three and two tiles; k = 3 (98 325 rows): four
and three -- both parities twice.  Every case asserts the tiles per wave it was built for.

1. Parity with oracle.svi.logreg_loglik at tests/test_bbvi_gpu.py's bound, unchanged, at S = 64: D = 256 and D = 64 on
   the default context (f32 DMA kernel, FULL and column-masked), the same two with two bf16 terms (bx kernel), and
   D = 256 with option bbvi_kernel = 2 (xreg kernel, which shares the draws' fill with the f32 DMA kernel).
2. Exact row accounting at k = 2 on the three routes: test_bbvi_gpu.test_loglik_operand_layout_with_exact_integers'
   construction (one-hot X, draws of 40, intercepts -20, y = 1) at its rtol of 1e-6.  Every logit is +20 or -20, a row
   adds -log(1 + e^-20) or -20 - log(1 + e^-20), so a lost or doubled row moves ell_s by 20 of about 20 N: 1.5e-5
   relative at 256 CUs.  The hot column is 7 n mod (256 >> sweep of n), so that the tiles a wave runs one after the
   other differ in their hits per sample: with every wave's second tile replaced by its first, every ell_s moves by
   more than 100 x the tolerance (asserted in exact_inputs; up to 1964 x at 256 CUs).  What this case does not see is stale y, ids or
   intercepts (they are constant or repeat with the sweep); those are held by the parity cases alone.
   Both sides sum in float64, so the per-row error does not grow with N.  Evaluated on the CPU in float32 terms with a
   float64 sum, as the kernels add them (in float32 1 + e^-20 is 1, every term is exactly 0 or -20), N = 65 557: worst
   |ell - oracle| / (1e-6 |oracle|) = 1.04e-4 over the 64 samples -- the 2.06e-9 per row that float32 drops, four
   orders inside the tolerance and 1.5e5 times smaller than one row.
3. Two calls at k = 2 are bit-equal on each route.

gemm_skinny_nt_kernel, which takes its ring from the same bsc_line_ring (csrc/bsc_common.h), already runs six tiles
per wave in tests/test_algebra_gpu.py::test_skinny_products_one_tiny_extent_nt[8-100003-256]: 6 251 tiles of 16 rows
(the last of 3) on 4 * 256 waves, K = 256, M = 8, against float64 and against the tile GEMM; no NT case is added here.
"""
import functools
import math

import numpy as np
import numpy.testing as npt
import pytest

from oracle import svi
from test_bbvi_gpu import _loglik
from test_mfma_split_gpu import split_ctx  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

XT, XW, S = 16, 8, 64              # csrc/bsc_bbvi.hip: rows per tile, waves per workgroup; config 5's draws
ROUTES = ("f32", "bx", "xreg")


def grid(N, cu):
    """bsc_logreg_bbvi_loglik's launch: -> n_tiles, n_waves, n_iter, the most and the fewest tiles of a wave."""
    n_tiles = (N + XT - 1) // XT
    n_blocks = max(1, min(cu, (n_tiles + XW - 1) // XW))
    n_waves = XW * n_blocks
    it = (n_tiles + n_waves - 1) // n_waves
    return n_tiles, n_waves, it + (it & 1), it, n_tiles // n_waves


def rows_for(k, cu):
    """k full sweeps of the grid, one full tile and a ragged one of five rows."""
    N = k * (XW * cu * XT) + XT + 5
    n_tiles, n_waves, n_iter, most, fewest = grid(N, cu)
    assert (n_waves, most, fewest) == (XW * cu, k + 1, k), (N, cu, n_waves, most, fewest)
    assert n_tiles - fewest * n_waves == 2 and N - XT * (n_tiles - 1) == 5      # two waves run k + 1; the last tile holds 5 rows
    assert n_iter == k + 1 + ((k + 1) & 1) and n_iter >= most
    return N


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.fixture(scope="module")
def xreg(ctx):
    from bayesic_amd.device import Context
    c = Context(ctx.device_index, stream=ctx.stream, options=dict(bbvi_kernel=2))
    yield c
    c.close()


def _on(route, ctx, xreg, split_ctx):
    """The context that runs `route`; the split setting is undone by the fixture."""
    if route == "bx":
        split_ctx(2)
    return xreg if route == "xreg" else ctx


@functools.lru_cache(maxsize=4)
def _inputs(N, D, G=37):
    """test_bbvi_gpu.test_loglik_matches_oracle's inputs, with the oracle's ell and the bound's sum(|l| + 1)."""
    rs = np.random.RandomState(N % 100000 + D + G)
    X = rs.standard_normal((N, D)).astype(np.float32)
    g = rs.randint(G, size=N).astype(np.int32)
    y = (rs.uniform(size=N) < 0.4).astype(np.float32)
    Wz = (rs.standard_normal((S, D)) / math.sqrt(D)).astype(np.float32)
    Bz = rs.standard_normal((G, S)).astype(np.float32)
    want = svi.logreg_loglik(X, y, g, Wz, Bz)
    bound = np.zeros(S)
    for i in range(0, N, 32768):
        bound += (np.abs(X[i:i + 32768].astype(np.float64) @ Wz.astype(np.float64).T + Bz.astype(np.float64)[g[i:i + 32768]])
                  + 1.0).sum(axis=0)
    return X, y, g, Wz, Bz, want, bound


@functools.lru_cache(maxsize=1)
def exact_inputs(N, sweep, D=256, G=4):
    """test_loglik_operand_layout_with_exact_integers at N rows: row n has a single 1, sample s looks at column 5 s mod D
    through a draw of 40, every intercept is -20, y = 1.  The hot column is 7 n mod (D >> (n // sweep)), sweep = the
    rows of one pass of the grid: with 7 n mod D alone every tile of a wave would hold the same X as the one before
    (7 * 128 cu mod 256 = 0 for even cu), and a ring slot still holding the previous tile would give the same sums.
    Here the k-th tile of every wave spreads its ones over D >> k columns, so the hits per sample differ from tile to
    tile and a stale X moves ell_s by thousands of rows.  (y, the ids and the intercepts are constant or repeat:
    stale side data is left to the random-data parity cases.)"""
    n = np.arange(N)
    col, look = (n * 7) % (D >> (n // sweep)), (np.arange(S) * 5) % D
    X = np.zeros((N, D), np.float32)
    X[n, col] = 1.0
    Wz = np.zeros((S, D), np.float32)
    Wz[np.arange(S), look] = 40.0
    Bz = np.full((G, S), -20.0, np.float32)
    g = (n % G).astype(np.int32)
    y = np.ones(N, np.float32)
    want = svi.logreg_loglik(X, y, g, Wz, Bz)
    # every wave's second tile read as its first again: each ell_s moves by 20 per hit won or lost, far past the rtol
    hits = [np.bincount(col[k * sweep:(k + 1) * sweep], minlength=D)[look] for k in (0, 1)]
    assert (20.0 * np.abs(hits[1] - hits[0]) > 100 * 1e-6 * np.abs(want)).all()
    return X, y, g, Wz, Bz, want


@pytest.mark.parametrize("route,D", [("f32", 256), ("f32", 64), ("bx", 256), ("bx", 64), ("xreg", 256)])
@pytest.mark.parametrize("k", [2, 3])
def test_loglik_matches_oracle_at_three_and_four_tiles_per_wave(ctx, xreg, split_ctx, cu, k, route, D):
    N = rows_for(k, cu)
    X, y, g, Wz, Bz, want, bound = _inputs(N, D)
    ell = _loglik(_on(route, ctx, xreg, split_ctx), X, y, g, Wz, Bz)
    err = np.abs(ell - want)
    print("bbvi loglik %s N=%d D=%d (%d and %d tiles per wave): worst err / (2e-5 bound) %.3g, err / |ell| %.3g" % (
        route, N, D, k + 1, k, (err / (2e-5 * bound)).max(), (err / np.abs(want)).max()))
    assert (err <= 2e-5 * bound + 1e-9).all(), (err / bound).max()


@pytest.mark.parametrize("route", ROUTES)
def test_loglik_counts_every_row_once(ctx, xreg, split_ctx, cu, route):
    N = rows_for(2, cu)
    X, y, g, Wz, Bz, want = exact_inputs(N, XW * cu * XT)
    assert len(set(np.round(want, 3))) > 1 and 20.0 / np.abs(want).max() > 5e-6      # one row is >= 5 x the tolerance
    ell = _loglik(_on(route, ctx, xreg, split_ctx), X, y, g, Wz, Bz)
    print("bbvi exact rows %s N=%d: worst |ell - oracle| / (1e-6 |oracle|) %.3g; one row is %.3g" % (
        route, N, (np.abs(ell - want) / (1e-6 * np.abs(want))).max(), (20.0 / (1e-6 * np.abs(want))).min()))
    npt.assert_allclose(ell, want, rtol=1e-6)


@pytest.mark.parametrize("route", ROUTES)
def test_two_calls_are_bit_equal(ctx, xreg, split_ctx, cu, route):
    X, y, g, Wz, Bz, _, _ = _inputs(rows_for(2, cu), 256)
    c = _on(route, ctx, xreg, split_ctx)
    npt.assert_array_equal(_loglik(c, X, y, g, Wz, Bz), _loglik(c, X, y, g, Wz, Bz))
