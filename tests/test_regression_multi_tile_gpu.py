"""The regression passes where a resident wave runs SEVERAL tiles (n_iter >= 2): csrc/bsc_glm.hip (glm_pass_kernel,
glm_pass_mfma_kernel), csrc/bsc_predict.hip (predict_kernel) and csrc/bsc_softmax.hip (softmax_pass_kernel,
softmax_predict_kernel) against the float64 restatements in tests/_glm_ref.py, tests/_predict_ref.py and
tests/_softmax_ref.py.  Every other GPU test of these kernels stops at one tile per wave (or two, once).

Shapes come from the device.  `grid` restates the host arithmetic of pass_grid (csrc/bsc_glm.hip:651-665,
csrc/bsc_softmax.hip:432-446) and of bsc_predict_pass (csrc/bsc_predict.hip:360-365): max_waves = 8 CUs,
n_iter = ceil(n_tiles / max_waves), waves = ceil(n_tiles / n_iter).  With cap = 8 CUs * rows_per_tile the batch for
n_iter tiles per wave is `rows_for` = (n_iter - 1) cap + rows_per_tile + 5: one full tile and a ragged one of five
rows beyond n_iter - 1 full sweeps.  Because the grid is re-balanced (waves = ceil(n_tiles / n_iter)), the last
iteration is then nearly full: at 256 CUs and 16-row tiles, B = 65 557 is 4 098 tiles on 1 366 waves (342 workgroups of
four, so 1 368 slots), and the third iteration holds 1 361 full tiles, the ragged one and six empty slots.  Every case
asserts the n_iter it was built for; tests/test_regression_multi_tile_cpu.py checks the table at 256 CUs.

1. Parity at n_iter >= 2 on the inputs of the existing tests (their `_inputs`, imported) at their tolerances, unchanged:
   test_glm_gpu._check_pass's (ell 2e-5 * sum(|y l| + A + 1); G rtol 1e-4, atol 1e-4 max|G|), test_predict_gpu._check's
   (_predict_ref.bounds), test_softmax_regression_gpu._assert_pass and _softmax_ref.predict_bounds.  The predictive
   outputs carry 64 sentinel elements past B whose bits must not change.
   bsc_softmax_predict_pass: _softmax_ref.predict costs 30 s at B = 65 557, K = 16, S = 64 (an einsum without BLAS), so
   where S K > 128 the per-row outputs are compared on `probe_rows` -- every 13th row (at least one row of every 16-row
   tile), plus every row of the first two and the last four tiles -- and ALL rows are held to: probabilities summing to
   one, lpd == 0 exactly where the label is outside [0, K), and lpd_sum equal to the float64 sum of the device's own lpd
   (the kernel adds exactly those).  The reference is per row, so the subset sees the same reference values.
2. Exact row accounting: W = 0, one-hot X with the hot column (5 n + n // 16) mod D, pseudo-random labels.  Every
   logit is 0, the Poisson residual is the integer y - 1, the logistic one y - 1/2, the softmax one 1[y = k] - 1/K:
   G is a sum of multiples of 1/16 far below 2^24 and a lost, doubled or mis-paired row moves an entry by >= 1/16
   (>= 1/2 for the GLM links).  Poisson: bit equality with the integer reference, ell == -B.  Logistic and softmax:
   bit equality too if a one-tile control (B = 16, same construction) is bit-exact, else (rows per column) * 2^-23.
   The predictive passes on the same inputs: every row 1/K and -log K, 1/2, 1 and -1 - lgamma(y + 1).
3. Determinism of the five entry points at n_iter = 3; bsc_glm_pass_update against bsc_glm_data_pass ->
   bsc_glm_update(stats) bit for bit at B = cap + 21; two GLMReparamSVI steps against _glm_ref.glm_step.

n_iter reached per entry point at 256 CUs: bsc_glm_data_pass 2, 3 (MFMA kernel) and 3, 4, 5 (eight-row kernel, both
FULL variants); bsc_predict_pass 2, 3; bsc_softmax_data_pass 3; bsc_softmax_predict_pass 2, 3; bsc_glm_pass_update 2.

NOT YET RUN ON A DEVICE.  This module was written and checked without a GPU: its own logic (shapes, references,
sentinels, the exact-accounting expectations) passes against a float64 stand-in for the five entry points, and the
float32 CPU evaluation in tests/test_regression_multi_tile_cpu.py is inside every borrowed bound.  The worst
error / bound per entry point (each case prints its own: run with -s) and whether the logistic and softmax exact cases
hold bit for bit or fall back to (rows per column) * 2^-23 are to be recorded here after the first device run.
"""
import functools
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch
from scipy.special import gammaln

import _glm_ref as glm
import _predict_ref as pref
import _softmax_ref as sref
import test_glm_gpu as glm_t
import test_predict_gpu as predict_t
import test_softmax_regression_gpu as softmax_t

pytestmark = pytest.mark.gpu

LINKS = ("logistic", "poisson")
MFMA_ROWS, VALU_ROWS = 16, 8          # csrc/bsc_glm.hip: MT_ROWS, ROWS; predict and softmax tiles are 16 rows
GUARD = 64                            # sentinel elements past B
SENTINEL = -777.0


# ---- 0. the grid ------------------------------------------------------------------------------------------------

def grid(B, rows, cu, waves_per_block=4):
    """pass_grid (csrc/bsc_glm.hip:651-665, csrc/bsc_softmax.hip:432-446; four waves per workgroup) and the inline
    copy in bsc_predict_pass (csrc/bsc_predict.hip:360-365; eight)."""
    n_tiles = (B + rows - 1) // rows
    max_waves = 2 * 4 * cu
    if n_tiles <= 0:
        return dict(n_tiles=0, n_iter=0, waves=0, n_blocks=1)
    n_iter = (n_tiles + max_waves - 1) // max_waves
    waves = (n_tiles + n_iter - 1) // n_iter
    return dict(n_tiles=n_tiles, n_iter=n_iter, waves=waves, n_blocks=(waves + waves_per_block - 1) // waves_per_block)


def rows_for(n_iter, rows, cu):
    """The smallest batch of the issue's form with n_iter tiles per wave: (n_iter - 1) cap + one tile + 5 rows."""
    return (n_iter - 1) * 8 * cu * rows + rows + 5


def batch(cu, n_iter, rows, waves_per_block=4):
    B = rows_for(n_iter, rows, cu)
    g = grid(B, rows, cu, waves_per_block)
    assert g["n_iter"] == n_iter, "B=%d on %d CUs gives n_iter=%d, wanted %d" % (B, cu, g["n_iter"], n_iter)
    assert B % rows == 5 and g["n_blocks"] > 1
    return B


def probe_rows(B):
    """Every 13th row (13 < 16: at least one row of every tile) and all rows of the first two and last four tiles."""
    return np.unique(np.concatenate([np.arange(0, B, 13), np.arange(min(32, B)), np.arange(max(B - 64, 0), B)]))


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


_glm_inputs = functools.lru_cache(maxsize=4)(glm_t._inputs)
_predict_inputs = functools.lru_cache(maxsize=4)(predict_t._inputs)
_softmax_inputs = functools.lru_cache(maxsize=4)(softmax_t._inputs)


def _guarded(ctx, shape, dtype=torch.float32):
    n = int(np.prod(shape)) + GUARD
    return torch.full((n,), SENTINEL, dtype=dtype, device=ctx.device)


def _guard_untouched(buf, n):
    tail = buf[n:].cpu().numpy()
    assert tail.size == GUARD
    npt.assert_array_equal(tail.view(np.int32), np.full(GUARD, SENTINEL, np.float32).view(np.int32))


# ---- runners ----------------------------------------------------------------------------------------------------

def _glm_pass(ctx, link, X, y, W, y_offset=False):
    B, D = X.shape
    S = W.shape[0]
    yd = ctx.to_device(np.concatenate([[9.0], y]).astype(np.float32))[1:] if y_offset else ctx.to_device(y)
    if D == 256:
        assert (yd.data_ptr() % 16 == 0) != y_offset      # which kernel runs (pass_rows, csrc/bsc_glm.hip:648)
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    ctx.call("bsc_glm_data_pass", glm_t.CODE[link], ctx.to_device(X), D, yd, B, D, ctx.to_device(W), S, ell, G)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy()


def _glm_assert(link, ell, G, X, y, W, tag=""):
    """test_glm_gpu._check_pass's assertions, restated for results that are already on the host."""
    ell_r, G_r = glm.glm_data_pass(link, X, y, W)
    L = X.astype(np.float64) @ W.astype(np.float64).T
    if link == "poisson":
        assert np.abs(L).max() <= 4.0
    A, _ = glm.log_partition(link, L)
    bound = (np.abs(y.astype(np.float64)[:, None] * L) + A + 1.0).sum(axis=0)
    err = np.abs(ell - ell_r)
    print("glm_pass %s%s B=%d D=%d S=%d: ell err/bound %.3g, G err/bound %.3g" % (
        link, tag, X.shape[0], X.shape[1], W.shape[0], (err / (2e-5 * bound)).max(),
        (np.abs(G - G_r) / (1e-4 * np.abs(G_r) + 1e-4 * np.abs(G_r).max())).max()))
    assert (err <= 2e-5 * bound + 1e-12).all(), (err / (bound + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())


def _predict(ctx, family, X, y, W, logvar):
    B, D = X.shape
    S = W.shape[0]
    out = {k: _guarded(ctx, B) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), SENTINEL, dtype=torch.float64, device=ctx.device)
    lvd = None if logvar is None else ctx.to_device(logvar)
    ctx.call("bsc_predict_pass", pref.CODE[family], ctx.to_device(X), D, ctx.to_device(y), B, D, ctx.to_device(W), lvd, S,
             out["mean"], out["var"], out["lpd"], out["lpd_sum"])
    ctx.sync()
    for k in ("mean", "var", "lpd"):
        _guard_untouched(out[k], B)
    return {k: v.cpu().numpy()[:B if k != "lpd_sum" else 1] for k, v in out.items()}


def _predict_assert(family, got, X, y, W, logvar, tag=""):
    """test_predict_gpu._check's assertions."""
    want = pref.predict(family, X, W, logvar, y)
    bnd = pref.bounds(family, X, W, logvar, y)
    if family == "poisson":
        assert np.abs(pref.logits(X, W)).max() <= 4.0
    worst = {k: float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300))) for k in ("mean", "var", "lpd", "lpd_sum")}
    print("predict_pass %s%s B=%d D=%d S=%d: worst error / bound  mean %.3g  var %.3g  lpd %.3g  lpd_sum %.3g" % (
        family, tag, X.shape[0], X.shape[1], W.shape[0], worst["mean"], worst["var"], worst["lpd"], worst["lpd_sum"]))
    for k, w in worst.items():
        assert w <= 1.0, (k, w)
    return want


def _softmax_predict(ctx, X, W, y):
    B, D = X.shape
    S, K = W.shape[:2]
    prob, lpd = _guarded(ctx, B * K), _guarded(ctx, B)
    lpd_sum = torch.full((1,), SENTINEL, dtype=torch.float64, device=ctx.device)
    ctx.call("bsc_softmax_predict_pass", ctx.to_device(X), D, ctx.to_device(np.asarray(y, np.int32)), B, D, K,
             ctx.to_device(W), S, prob, lpd, lpd_sum)
    ctx.sync()
    _guard_untouched(prob, B * K)
    _guard_untouched(lpd, B)
    return dict(prob=prob.cpu().numpy()[:B * K].reshape(B, K), lpd=lpd.cpu().numpy()[:B], lpd_sum=lpd_sum.cpu().numpy())


# ---- 1. parity at n_iter >= 2 -----------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [8, 9])
@pytest.mark.parametrize("n_iter", [2, 3])
@pytest.mark.parametrize("link", LINKS)
def test_glm_pass_mfma_kernel(ctx, cu, link, n_iter, S):
    """D = 256, y aligned: glm_pass_mfma_kernel.  S = 9: a second launch reuses the slab."""
    B = batch(cu, n_iter, MFMA_ROWS)
    X, y, W = _glm_inputs(link, B, 256, S, n_iter)
    _glm_assert(link, *_glm_pass(ctx, link, X, y, W), X, y, W)


@pytest.mark.parametrize("D,n_iter", [(64, 3), (64, 4), (64, 5), (252, 3)])
@pytest.mark.parametrize("link", LINKS)
def test_glm_pass_eight_row_kernel(ctx, cu, link, D, n_iter):
    """glm_pass_kernel<., false>: an odd tail after one ping-pong trip (3), two full trips (4), an odd tail after two
    (5)."""
    B = batch(cu, n_iter, VALU_ROWS)
    X, y, W = _glm_inputs(link, B, D, 8, n_iter)
    _glm_assert(link, *_glm_pass(ctx, link, X, y, W), X, y, W)


def test_glm_pass_eight_row_kernel_at_full_width(ctx, cu):
    """D = 256 with y 4 bytes into its buffer: glm_pass_kernel<., true> at n_iter = 3."""
    B = batch(cu, 3, VALU_ROWS)
    X, y, W = _glm_inputs("logistic", B, 256, 8, 3)
    _glm_assert("logistic", *_glm_pass(ctx, "logistic", X, y, W, y_offset=True), X, y, W, tag=" (y offset)")


@pytest.mark.parametrize("S", [8, 17, 64])            # NC = 1, 2, 4
@pytest.mark.parametrize("n_iter", [2, 3])
@pytest.mark.parametrize("family", pref.FAMILIES)
def test_predict_pass_full_width(ctx, cu, family, n_iter, S):
    B = batch(cu, n_iter, MFMA_ROWS, waves_per_block=8)
    X, y, W, logvar = _predict_inputs(family, B, 256, S, n_iter)
    _predict_assert(family, _predict(ctx, family, X, y, W, logvar), X, y, W, logvar)


@pytest.mark.parametrize("D", [252, 64])              # two strips, not FULL; one strip
@pytest.mark.parametrize("family", pref.FAMILIES)
def test_predict_pass_narrow(ctx, cu, family, D):
    B = batch(cu, 3, MFMA_ROWS, waves_per_block=8)
    X, y, W, logvar = _predict_inputs(family, B, D, 8, 3)
    _predict_assert(family, _predict(ctx, family, X, y, W, logvar), X, y, W, logvar)


@pytest.mark.parametrize("K,D", [(2, 256), (5, 256), (16, 256), (3, 64)])
def test_softmax_pass(ctx, cu, K, D):
    B = batch(cu, 3, MFMA_ROWS)
    X, y, W = _softmax_inputs(B, D, K, 16 // K + 1, K)       # two launches
    ell, G = softmax_t._pass(ctx, X, y, W)
    softmax_t._assert_pass(ell, G, X, y, W, tag="softmax_pass")


@pytest.mark.parametrize("S", [1, 7, 64])             # one draw group; several groups re-read per tile
@pytest.mark.parametrize("n_iter", [2, 3])
@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("K", [3, 16])
def test_softmax_predict_pass(ctx, cu, K, D, n_iter, S):
    B = batch(cu, n_iter, MFMA_ROWS)
    X, y, W = _softmax_inputs(B, D, K, S, K + n_iter)
    y = y.copy()
    y[::9] = -1 if K == 3 else K                      # rows with a label outside the classes score 0
    out = _softmax_predict(ctx, X, W, y)
    rows = np.arange(B) if S * K <= 128 else probe_rows(B)
    r, b = sref.predict(X[rows], W, y[rows]), sref.predict_bounds(X[rows], W, y[rows])
    perr, lerr = np.abs(out["prob"][rows] - r["prob"]), np.abs(out["lpd"][rows] - r["lpd"])
    print("softmax_predict B=%d K=%d D=%d S=%d (%d rows compared): prob err/bound %.3g, lpd err/bound %.3g" % (
        B, K, D, S, rows.size, (perr / b["prob"]).max(), (lerr / (b["lpd"] + 1e-300)).max()))
    assert (perr <= b["prob"]).all()
    assert (lerr <= b["lpd"]).all()
    # every row
    assert (out["lpd"][::9] == 0.0).all()
    assert np.abs(out["prob"].astype(np.float64).sum(axis=1) - 1.0).max() <= K * 1e-6
    dev_sum = out["lpd"].astype(np.float64).sum()
    assert abs(out["lpd_sum"][0] - dev_sum) <= 1e-12 * abs(dev_sum)
    if rows.size == B:
        assert abs(out["lpd_sum"][0] - r["lpd_sum"]) <= b["lpd_sum"]


# ---- 2. exact row accounting ------------------------------------------------------------------------------------

def exact_inputs(B, D, n_values, seed):
    """One-hot X (hot column (5 n + n // 16) mod D) and pseudo-random integer labels in [0, n_values)."""
    n = np.arange(B)
    col = (5 * n + n // 16) % D
    X = np.zeros((B, D), np.float32)
    X[n, col] = 1.0
    return X, col, np.random.RandomState(seed).randint(0, n_values, size=B)


def column_sums(col, values, D):
    """sum_{n: col(n) = c} values[n] in float64: exact for multiples of 1/16 this small."""
    return np.bincount(col, weights=values, minlength=D)


def _exact_or_ulp(name, G, G_r, G_ctl, G_ctl_r, per_col):
    if np.array_equal(G_ctl, G_ctl_r):
        print("%s: the one-tile control is bit-exact; bit equality required" % name)
        npt.assert_array_equal(G, G_r)
    else:
        print("%s: the one-tile control is NOT bit-exact; (rows per column) * 2^-23" % name)
        assert np.abs(G - G_r).max() <= per_col * 2.0 ** -23


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("link", LINKS)
def test_glm_pass_counts_every_row_once(ctx, cu, link, D):
    S = 8
    B = batch(cu, 3, MFMA_ROWS if D == 256 else VALU_ROWS)
    X, col, y = exact_inputs(B, D, 4 if link == "poisson" else 2, seed=D)
    W = np.zeros((S, D), np.float32)
    y32 = y.astype(np.float32)
    shift = 1.0 if link == "poisson" else 0.5
    G_r = np.tile(column_sums(col, y - shift, D), (S, 1))
    assert np.abs(G_r).max() < 2 ** 20 and len(np.unique(G_r)) >= 4
    ell, G = _glm_pass(ctx, link, X, y32, W)
    if link == "poisson":
        npt.assert_array_equal(G, G_r)
        npt.assert_array_equal(ell, np.full(S, -float(B)))
    else:
        Xc, colc, yc = exact_inputs(16, D, 2, seed=D)
        _, G_ctl = _glm_pass(ctx, link, Xc, yc.astype(np.float32), W)
        _exact_or_ulp("glm logistic D=%d" % D, G, G_r, G_ctl, np.tile(column_sums(colc, yc - 0.5, D), (S, 1)),
                      np.bincount(col).max())
        ulp = float(np.spacing(np.float32(math.log(2.0))))
        print("glm logistic D=%d: |ell + B log 2| / (B ulp) %.3g" % (D, np.abs(ell + B * math.log(2.0)).max() / (B * ulp)))
        assert np.abs(ell + B * math.log(2.0)).max() <= B * ulp


def _softmax_exact_G(col, y, K, D, S):
    G = np.stack([column_sums(col, (y == k) - 1.0 / K, D) for k in range(K)])
    return np.tile(G[None], (S, 1, 1))


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("K", [2, 4, 16])
def test_softmax_pass_counts_every_row_once(ctx, cu, K, D):
    S = 16 // K + 1
    B = batch(cu, 3, MFMA_ROWS)
    X, col, y = exact_inputs(B, D, K, seed=K + D)
    W = np.zeros((S, K, D), np.float32)
    G_r = _softmax_exact_G(col, y, K, D, S)
    assert len(np.unique(G_r)) >= 4
    ell, G = softmax_t._pass(ctx, X, y, W)
    Xc, colc, yc = exact_inputs(16, D, K, seed=K + D)
    _, G_ctl = softmax_t._pass(ctx, Xc, yc, W)
    _exact_or_ulp("softmax K=%d D=%d" % (K, D), G, G_r, G_ctl, _softmax_exact_G(colc, yc, K, D, S), np.bincount(col).max())
    ulp = float(np.spacing(np.float32(math.log(K))))
    print("softmax K=%d D=%d: |ell + B log K| / (B ulp) %.3g" % (K, D, np.abs(ell + B * math.log(K)).max() / (B * ulp)))
    assert np.abs(ell + B * math.log(K)).max() <= B * ulp


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("family", ["logistic", "poisson"])
def test_predict_pass_pairs_every_row_with_its_own_y(ctx, cu, family, D):
    S = 8
    B = batch(cu, 3, MFMA_ROWS, waves_per_block=8)
    X, col, y = exact_inputs(B, D, 4 if family == "poisson" else 2, seed=D + 1)
    y32 = y.astype(np.float32)
    W = np.zeros((S, D), np.float32)
    got = _predict(ctx, family, X, y32, W, None)
    want = _predict_assert(family, got, X, y32, W, None, tag=" (W = 0)")
    if family == "poisson":
        npt.assert_allclose(want["mean"], 1.0, rtol=1e-15)
        npt.assert_allclose(want["lpd"], -1.0 - gammaln(y + 1.0), rtol=1e-14)
    else:
        npt.assert_allclose(want["mean"], 0.5, rtol=1e-15)
        npt.assert_allclose(want["lpd"], -math.log(2.0), rtol=1e-14)


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("K", [2, 4, 16])
def test_softmax_predict_pass_scores_every_row(ctx, cu, K, D):
    """prob = 1/K and lpd = -log K in every row (0 where the label is outside the classes), at the closed forms of
    _softmax_ref.predict_bounds for W = 0 (a = 0): prob 2e-5 / K, lpd 2 * 2e-5 (log K + 1)."""
    S = 16 // K + 1
    B = batch(cu, 3, MFMA_ROWS)
    X, col, y = exact_inputs(B, D, K, seed=K + D + 1)
    y[::9] = np.where(np.arange(y[::9].size) % 2 == 0, -1, K)
    W = np.zeros((S, K, D), np.float32)
    out = _softmax_predict(ctx, X, W, y)
    r, b = sref.predict(X[:64], W, y[:64]), sref.predict_bounds(X[:64], W, y[:64])       # the closed forms are the reference's
    ok = sref.valid_rows(y, K)
    npt.assert_allclose(r["prob"], 1.0 / K, rtol=1e-15)
    npt.assert_allclose(r["lpd"], np.where(ok[:64], -math.log(K), 0.0), rtol=1e-15)
    npt.assert_allclose(b["prob"], sref.EPS / K, rtol=1e-12)
    npt.assert_allclose(b["lpd"], np.where(ok[:64], 2.0 * sref.EPS * (math.log(K) + 1.0), 0.0), rtol=1e-12)
    assert np.abs(out["prob"] - 1.0 / K).max() <= sref.EPS / K
    lpd_r = np.where(ok, -math.log(K), 0.0)
    assert (np.abs(out["lpd"] - lpd_r) <= np.where(ok, 2.0 * sref.EPS * (math.log(K) + 1.0), 0.0)).all()
    assert abs(out["lpd_sum"][0] - lpd_r.sum()) <= ok.sum() * 2.0 * sref.EPS * (math.log(K) + 1.0)


# ---- 3. determinism, the one-call update, the driver --------------------------------------------------------------

def _same(a, b):
    for u, v in zip(a, b):
        npt.assert_array_equal(u, v)


def test_two_runs_are_byte_identical(ctx, cu):
    B16, B8 = batch(cu, 3, MFMA_ROWS), batch(cu, 3, VALU_ROWS)
    X, y, W = _glm_inputs("poisson", B16, 256, 9, 3)
    _same(_glm_pass(ctx, "poisson", X, y, W), _glm_pass(ctx, "poisson", X, y, W))
    X, y, W = _glm_inputs("logistic", B8, 64, 8, 3)
    _same(_glm_pass(ctx, "logistic", X, y, W), _glm_pass(ctx, "logistic", X, y, W))
    X, y, W, logvar = _predict_inputs("gaussian", B16, 256, 17, 3)
    a, b = _predict(ctx, "gaussian", X, y, W, logvar), _predict(ctx, "gaussian", X, y, W, logvar)
    _same([a[k] for k in sorted(a)], [b[k] for k in sorted(b)])
    X, y, W = _softmax_inputs(B16, 256, 5, 4, 5)
    _same(softmax_t._pass(ctx, X, y, W), softmax_t._pass(ctx, X, y, W))
    X, y, W = _softmax_inputs(B16, 64, 3, 7, 6)
    a, b = _softmax_predict(ctx, X, W, y), _softmax_predict(ctx, X, W, y)
    _same([a[k] for k in sorted(a)], [b[k] for k in sorted(b)])


@pytest.mark.parametrize("link", LINKS)
def test_one_call_update_equals_pass_then_update(ctx, cu, link):
    """bsc_glm_pass_update against bsc_glm_data_pass -> bsc_glm_update(stats) on identical state, two tiles per wave:
    the same pass kernel, the same slab, float64 sums of float32 partials that are exact in either order."""
    D, S, seed, t, scale, tau, lr = 256, 8, 99, 4, 12.5, 0.7, 0.02
    B = batch(cu, 2, MFMA_ROWS)
    assert B == 8 * cu * MFMA_ROWS + 21
    X, y = glm_t._regression_data(link, B, D, 3)
    rs = np.random.RandomState(B % 1000)
    f64 = torch.float64
    lam = np.concatenate([0.05 * rs.standard_normal(D), math.log(0.1) + 0.1 * rs.standard_normal(D)])
    m1, m2 = 0.01 * rs.standard_normal(2 * D), 1e-4 * rs.uniform(size=2 * D)
    eps, eps_n = np.zeros((S, D + 1)), np.zeros((S, D + 1))
    eps[:, :D], eps_n[:, :D] = glm.noise(D, S, seed, t - 1), glm.noise(D, S, seed, t)
    W = glm.draw(lam, eps[:, :D])
    Xd, yd = ctx.to_device(X), ctx.to_device(y)
    runs = []
    for one_call in (True, False):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * D, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W_n=ctx.zeros(S * D), elbo=ctx.zeros(1, f64),
                 grad=ctx.zeros(2 * D, f64))
        tail = (scale, tau, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["elbo"], d["grad"])
        if one_call:
            ctx.call("bsc_glm_pass_update", glm_t.CODE[link], Xd, D, yd, B, D, d["lam"], d["out"], d["m1"], d["m2"],
                     d["eps"], d["W"], S, *tail)
        else:
            stats = ctx.zeros(S * (D + 1), f64)
            ctx.call("bsc_glm_data_pass", glm_t.CODE[link], Xd, D, yd, B, D, d["W"], S, stats[:S], stats[S:])
            ctx.call("bsc_glm_update", stats, d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], D, S, *tail)
        ctx.sync()
        runs.append({k: d[k].cpu().numpy() for k in ("out", "m1", "m2", "elbo", "grad", "W_n")})
    for k in runs[0]:
        npt.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
    ell, G = glm.glm_data_pass(link, X, y, W)
    lam_r, _, _, elbo_r, grad_r = glm.finish(lam, m1, m2, t, eps[:, :D], W, ell, G, scale, tau, lr)
    npt.assert_allclose(runs[0]["elbo"][0], elbo_r, rtol=1e-6)
    assert np.abs(runs[0]["grad"] - grad_r).max() <= 1e-4 * np.abs(grad_r).max()
    npt.assert_allclose(runs[0]["out"], lam_r, atol=2e-4)


@pytest.mark.parametrize("link", LINKS)
def test_two_driver_steps_track_the_reference(ctx, cu, link):
    """test_glm_gpu.test_twenty_updates_track_the_reference_over_two_batches' tolerances at two tiles per wave."""
    from bayesic_amd.svi import GLMReparamSVI
    D, S, seed, lr, tau = 256, 8, 1234, 0.01, 2.0
    B = batch(cu, 2, MFMA_ROWS)
    X, y = glm_t._regression_data(link, B, D, 5)
    model = GLMReparamSVI(ctx.to_device(X), ctx.to_device(y), link=link, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr,
                          prior_precision=tau, ctx=ctx)
    lam = glm.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in (1, 2):
        assert model.step() is None
        lam, m1, m2, elbo, grad = glm.glm_step(link, lam, m1, m2, t, X, y, S, seed, 10.0 * B, lr, tau)
        ctx.sync()
        g = model.grad.cpu().numpy()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
