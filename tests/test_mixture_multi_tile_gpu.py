"""The mixture's local step where a wave (a workgroup) runs SEVERAL row tiles: bsc_mog_estep (csrc/bsc_mog.hip:
mog_estep_kernel<FULL, NT>, mog_estep_bx_kernel<FULL>), bsc_gemm_softmax_rows / bsc_gemm_softmax_stats
(csrc/bsc_rowsoftmax.hip) and bsc_weighted_outer (csrc/bsc_wouter.hip).  The older tests of these entry points stop at one
tile per wave (N <= 40 000 on 256 CUs), or reach more only at sizes where their bounds are wider than whole rows.

0. Shapes come from the device: tests/_mixture_ref.py restates the three host grids, and every case asserts the
   n_iter / iters it was built for.  With cap = 8 CUs * 32 rows: N = (it - 1) cap + 37 (one full tile and a ragged one of
   five rows beyond it - 1 sweeps; the re-balanced grid makes the last trip nearly full) and N = it cap - 27 (every wave
   slot used, the very last tile ragged).  At 256 CUs: 65 573, 131 109, 196 645, 262 181 rows and 131 045.
   tests/test_mixture_multi_tile_cpu.py checks the tables at 256 CUs.
1. bsc_mog_estep at it = 2, 3, 5 (n_iter = 2, 4, 6: both buffers hold real tiles; a trailing all-empty trip; three buffer
   pairs) on its five instantiations: <true, false> (D = 16), <true, true> (D = 16, option mog_nt = 1), <false, true>
   (D = 12 / K = 64 and D = 5 / K = 33, ldx > D, NaN in the padding), bx<true> and bx<false> (mfma_split = 2).
   (a) Exact row accounting on _mixture_ref.estep_exact_data: r is exactly one-hot, every float32 partial sum an integer
       below 2^24, so [R | S1 | S2] must EQUAL the int64 sums per label; a dropped, doubled or swapped tile changes an
       integer because labels and offsets are pseudo-random in the row.  On the split route counts and first moments must
       be bit-equal; the squares (x^2 < 2^16 fits two bf16 terms) too if the device gives it, else 2^-17 relative, and the
       case prints which.  mog_nt = 1 must equal mog_nt = 0 bit for bit.  lse of the same runs against the oracle at rtol
       2e-6, in a test of its own (it found the rounding of the pre-scaled coefficients: see the figures below).
   (b) Parity with oracle.svi.mog_local_step on test_mog_gpu.test_estep_matches_oracle's data at its tolerances,
       unchanged (2e-5 scale + 1e-9; sum R = N at rtol 1e-6; lse at rtol 2e-6), and run-to-run identity.
2. bsc_gemm_softmax_rows at raw n_iter 2 (-> 3) and 4 (-> 6: the second rotation of the three buffers), K = 40, N = 64,
   one transposed B: every row against float64 at test_softmax_gpu.test_gemm_softmax_rows_matches_numpy's tolerances; R,
   lse and cross carry 64 sentinel elements past `rows` whose bits must not change.  bsc_gemm_softmax_stats at raw n_iter
   2 and 3 (-> 4: a trailing all-empty trip), write_r both ways, a bias row once, at test_softmax_stats_gpu's tolerances.
   Exact accounting for both: B = 0, A integers in [-3, 3] -> every R is exactly 1/64, cross exactly 0, stats[c, f]
   exactly sum_rows A[row, f] / 64, lse_sum = rows log 64 at rtol 2e-6; bit equality on R and stats.
3. bsc_weighted_outer at iters = 2 and 3: non-symmetric K = 32, D = E = 32 (KT = 1, gy = 4), non-symmetric K = 64, D = 16,
   E = 12 (KT = 2, gy = 2; once with padded leading dimensions) and symmetric K = 64, D = 16.  Exact: one-hot R with a
   pseudo-random hot column, integer X and Y, scale 1, array_equal with the int64 sums.  Parity: test_wouter_gpu's
   reference (as chunked matrix products, _mixture_ref.wouter_reference: its einsum takes 14 s at 65 605 rows; the CPU
   module holds the two together) and 2e-5 * bound on its kind of random data.

MEASURED ON AN MI355X (256 CUs), worst error / bound over the cases of each entry point (every case prints its own: -s).
 * bsc_mog_estep, exact accounting: all 20 cases bit-equal to the int64 sums, on the split route the squares too (bit-exact
   in all seven split cases); mog_nt = 1 equals mog_nt = 0 bit for bit.
 * bsc_mog_estep, lse ON THE EXACT DATA at rtol 2e-6 (test_estep_exact_data_lse_matches_oracle): equal to the oracle in all
   20 cases.  BUG FOUND AND FIXED: with W and c scaled by log2 e and rounded before the forward product, as the kernels
   did, this check failed in 13 of the 20 cases -- 1.64 to 1.66 x the tolerance on the split route at D = 16, 10.9 to
   11.0 x (split) and 16.2 to 16.4 x (f32) at D = 12, 42.9 to 43.1 x at D = 5 / K = 33 (0.14 to 0.32 on the f32 kernels at
   D = 16).  On these data a row's logit (about -5) is what is left of terms of up to 41 000 (log2 units: centre 168,
   x 170), so the coefficients' separate roundings, 2^-24 of each TERM, did not cancel: 4.3e-4 per row at D = 5, the same
   at it = 2, 3 and 5 -- the arithmetic, not the schedule (tests/test_mixture_multi_tile_cpu.py holds the float32 chain
   both ways).  The kernels now form the logits in natural units and multiply (l - m) by log2 e; at 10M x 16, K = 64
   (tools/bench_mog_split.py, profiles/mog_natural_logits_ab.txt) the pass takes 746.6 us against 745.9 before on the f32
   kernel and 507.2 against 502.3 on the split route, and lse moves from 7.3e-8 to 1.1e-9 of the float64 value.
 * bsc_mog_estep, parity: statistics 2.3e-4 of the bound on the f32 kernels (D = 5, it = 3), 8.5e-4 on the split route;
   sum R = N 2.3e-3 of its rtol; lse 9.2e-3 of its rtol (8.3e-2 before the fix).
 * bsc_gemm_softmax_rows: R 0.41, lse 0.030, cross 0.019, row sums 0.066 of their bounds; sentinels untouched; on zero
   logits R and cross bit-equal.  bsc_gemm_softmax_stats: statistics 0.049, lse_sum 0.031, R 0.36 of their bounds; on zero
   logits statistics and R bit-equal.
 * bsc_weighted_outer: 3.3e-3 of the bound (symmetric), 5.0e-4 (non-symmetric); the exact cases equal the int64 sums.
"""
import functools
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _mixture_ref as mr
from oracle import svi
from test_regression_multi_tile_gpu import _guard_untouched, _guarded   # 64 sentinel elements past the end
from test_mfma_split_gpu import split_ctx  # noqa: F401  (fixture: sets the split, resets it to 0 afterwards)
from test_wouter_gpu import run as wo_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.fixture(scope="module")
def nt_ctx(ctx):
    from bayesic_amd.device import Context
    c = Context(ctx.device_index, stream=ctx.stream, options=dict(mog_nt=1))
    assert c.get_option("mog_nt") == 1 and ctx.get_option("mog_nt") == 0
    yield c
    c.close()


def rows_for(form, it, cu):
    return mr.rows_rebalanced(it, cu) if form == "rebalanced" else mr.rows_full_grid(it, cu)


# ---- 1. bsc_mog_estep ---------------------------------------------------------------------------------------------

# route -> (D, K, ldx, split terms, which context)
ROUTES = {
    "f32": (16, 64, 16, 0, "default"),          # mog_estep_kernel<true, false>
    "f32_nt": (16, 64, 16, 0, "nt"),            # mog_estep_kernel<true, true>
    "masked_d12": (12, 64, 13, 0, "default"),   # mog_estep_kernel<false, true>, rows 52 bytes apart
    "masked_d5": (5, 33, 8, 0, "default"),      # mog_estep_kernel<false, true>, K < 64
    "bx": (16, 64, 16, 2, "default"),           # mog_estep_bx_kernel<true>
    "bx_d12": (12, 64, 13, 2, "default"),       # mog_estep_bx_kernel<false>
}
ESTEP_CASES = [(r, "rebalanced", it) for r in ROUTES for it in (2, 3, 5)] + [("f32", "full", 2), ("bx", "full", 2)]


def estep_rows(form, it, cu):
    N = rows_for(form, it, cu)
    g = mr.estep_grid(N, cu)
    assert g["it"] == it and g["n_iter"] == it + (it & 1), (N, cu, g)
    assert g["n_blocks"] > 1 and N % mr.MT == 5
    if form == "full":
        assert g["waves"] == 8 * cu and g["n_tiles"] == it * 8 * cu
    return N


def _estep(c, X, Wmat, cvec, ldx):
    N, D = X.shape
    K = Wmat.shape[0]
    if ldx == D:
        Xd = c.to_device(X)
    else:
        wide = np.full((N, ldx), np.nan, np.float32)          # the padding must never be read as data
        wide[:, :D] = X
        Xd = c.to_device(wide)
    Wd, cd = c.to_device(Wmat), c.to_device(cvec)
    stats, lse = c.zeros((K, 1 + 2 * D), torch.float64), c.zeros(1, torch.float64)
    c.call("bsc_mog_estep", Xd, ldx, N, D, K, Wd, cd, stats, lse)
    c.sync()
    return stats.cpu().numpy(), lse.item()


# inputs and references, computed once per shape and shared (nothing writes to them)
@functools.lru_cache(maxsize=2)
def _exact(N, K, D):
    X, Wmat, c, labels, want = mr.estep_exact_data(N, K, D)
    _, lse_ref = svi.mog_local_step(X, Wmat, c)
    return X, Wmat, c, want, lse_ref


@functools.lru_cache(maxsize=2)
def _overlap(N, D, K):
    X, Wmat, c = mr.estep_overlap_data(N, D, K)
    want, lse_ref = svi.mog_local_step(X, Wmat, c)
    scale = mr.estep_scale(X)
    return X, Wmat, c, want, lse_ref, scale


# sorted by shape, so that the cached inputs and references are shared by the routes that use them
ESTEP_SORTED = sorted(ESTEP_CASES, key=lambda t: (ROUTES[t[0]][:2], t[1], t[2]))


@pytest.mark.parametrize("route,form,it", ESTEP_SORTED)
def test_estep_exact_row_accounting(ctx, nt_ctx, split_ctx, cu, route, form, it):  # noqa: F811
    D, K, ldx, terms, which = ROUTES[route]
    N = estep_rows(form, it, cu)
    X, Wmat, c, want, lse_ref = _exact(N, K, D)
    if terms:
        split_ctx(terms)
    stats, lse = _estep(nt_ctx if which == "nt" else ctx, X, Wmat, c, ldx)
    npt.assert_array_equal(stats[:, :1 + D], want[:, :1 + D])
    if terms:
        exact_squares = np.array_equal(stats[:, 1 + D:], want[:, 1 + D:])
        print("mog_estep exact %s N=%d it=%d: squares on the split route %s" % (
            route, N, it, "bit-exact" if exact_squares else "NOT bit-exact, worst relative %.3g" % np.max(
                np.abs(stats[:, 1 + D:] - want[:, 1 + D:]) / np.maximum(want[:, 1 + D:], 1))))
        if not exact_squares:
            npt.assert_allclose(stats[:, 1 + D:], want[:, 1 + D:], rtol=2.0 ** -17)
    else:
        npt.assert_array_equal(stats[:, 1 + D:], want[:, 1 + D:])
    if which == "nt":                      # only the cache policy of the loads differs
        plain, lse_plain = _estep(ctx, X, Wmat, c, ldx)
        npt.assert_array_equal(stats, plain)
        assert lse == lse_plain


@pytest.mark.parametrize("route,form,it", ESTEP_SORTED)
def test_estep_exact_data_lse_matches_oracle(ctx, nt_ctx, split_ctx, cu, route, form, it):  # noqa: F811
    """The bound term on the exact data, at test_estep_matches_oracle's rtol 2e-6: in natural units every product and
    partial sum of the own component's logit is a half-integer below 2^24, so the kernels return the oracle's value.
    With coefficients scaled by log2 e beforehand this was up to 43 x the tolerance away (module docstring)."""
    D, K, ldx, terms, which = ROUTES[route]
    N = estep_rows(form, it, cu)
    X, Wmat, c, _, lse_ref = _exact(N, K, D)
    if terms:
        split_ctx(terms)
    _, lse = _estep(nt_ctx if which == "nt" else ctx, X, Wmat, c, ldx)
    print("mog_estep exact %s N=%d it=%d: lse relative error / 2e-6 = %.3g" % (
        route, N, it, abs(lse - lse_ref) / (2e-6 * abs(lse_ref))))
    npt.assert_allclose(lse, lse_ref, rtol=2e-6, atol=1e-4)


@pytest.mark.parametrize("route,form,it", [t for t in ESTEP_SORTED if t != ("bx", "full", 2)])
def test_estep_matches_oracle_at_several_tiles_per_wave(ctx, nt_ctx, split_ctx, cu, route, form, it):  # noqa: F811
    D, K, ldx, terms, which = ROUTES[route]
    N = estep_rows(form, it, cu)
    X, Wmat, c, want, lse_ref, scale = _overlap(N, D, K)
    if terms:
        split_ctx(terms)
    dev = nt_ctx if which == "nt" else ctx
    stats, lse = _estep(dev, X, Wmat, c, ldx)
    print("mog_estep parity %s N=%d it=%d: stats err / bound %.3g, sum R %.3g of 1e-6, lse %.3g of 2e-6" % (
        route, N, it, (np.abs(stats - want) / (2e-5 * scale[None, :] + 1e-9)).max(),
        abs(stats[:, 0].sum() - N) / (1e-6 * N), abs(lse - lse_ref) / (2e-6 * abs(lse_ref))))
    assert (np.abs(stats - want) <= 2e-5 * scale[None, :] + 1e-9).all(), \
        np.abs((stats - want) / scale[None, :]).max()
    npt.assert_allclose(stats[:, 0].sum(), N, rtol=1e-6, atol=1e-6)
    npt.assert_allclose(lse, lse_ref, rtol=2e-6, atol=1e-4)
    again, lse2 = _estep(dev, X, Wmat, c, ldx)
    npt.assert_array_equal(stats, again)
    assert lse == lse2
    if which == "nt":
        plain, lse_plain = _estep(ctx, X, Wmat, c, ldx)
        npt.assert_array_equal(stats, plain)
        assert lse == lse_plain


# ---- 2. bsc_gemm_softmax_rows / bsc_gemm_softmax_stats -------------------------------------------------------------

SK, SN = 40, 64                        # contraction extent and softmax columns


def softmax_rows_for(kernel, form, raw, cu):
    rows = rows_for(form, raw, cu)
    g = (mr.softmax_rows_grid if kernel == "rows" else mr.softmax_stats_grid)(rows, cu)
    want = (raw + 2) // 3 * 3 if kernel == "rows" else raw + (raw & 1)
    assert g["raw"] == raw and g["n_iter"] == want and g["n_blocks"] > 1, (rows, cu, g)
    assert rows % mr.MT == 5
    return rows


def _softmax_rows(ctx, A, lda, B, transposed_b, alpha):
    rows = A.shape[0]
    Ah = np.zeros((rows, lda), np.float32)
    Ah[:, :SK] = A
    Ad = ctx.to_device(Ah)
    Bd = ctx.to_device(np.ascontiguousarray(B.T)) if transposed_b else ctx.to_device(B)
    ldbk, ldbn = (1, SK) if transposed_b else (SN, 1)
    R, lse, cross = _guarded(ctx, rows * SN), _guarded(ctx, rows), _guarded(ctx, rows)
    ctx.call("bsc_gemm_softmax_rows", Ad, lda, rows, SK, Bd, ldbk, ldbn, SN, alpha, R, SN, lse, cross)
    ctx.sync()
    _guard_untouched(R, rows * SN)
    _guard_untouched(lse, rows)
    _guard_untouched(cross, rows)
    return R[:rows * SN].cpu().numpy().reshape(rows, SN), lse[:rows].cpu().numpy(), cross[:rows].cpu().numpy()


def _softmax_stats(ctx, A, lda, B, alpha, write_r, bias=None):
    """-> stats [SN, SK (+ 1)], lse_sum, R or None.  `bias`: row SK of B."""
    rows = A.shape[0]
    Ah = np.zeros((rows, lda), np.float32)
    Ah[:, :SK] = A
    Ad, Bd = ctx.to_device(Ah), ctx.to_device(B)
    cols = SK + (1 if bias else 0)
    stats = torch.full((SN, cols + 2), float("nan"), dtype=torch.float32, device=ctx.device)
    lse = torch.full((1,), float("nan"), dtype=torch.float64, device=ctx.device)
    R = _guarded(ctx, rows * SN) if write_r else None
    ctx.call("bsc_gemm_softmax_stats", Ad, lda, rows, SK, Bd, SN, 1, SN, alpha, Bd[SK] if bias else None, R, SN, stats,
             cols + 2, lse)
    ctx.sync()
    got = stats.cpu().numpy()
    assert np.isnan(got[:, cols:]).all()                                   # padding untouched
    if write_r:
        _guard_untouched(R, rows * SN)
    return got[:, :cols], lse.item(), (R[:rows * SN].cpu().numpy().reshape(rows, SN) if write_r else None)


@pytest.mark.parametrize("form,raw,transposed_b", [("rebalanced", 2, False), ("rebalanced", 4, False), ("full", 2, True),
                                                   ("rebalanced", 4, True)])
def test_gemm_softmax_rows_through_the_buffer_rotation(ctx, cu, form, raw, transposed_b):
    rows = softmax_rows_for("rows", form, raw, cu)
    rs = np.random.RandomState(rows + SK + SN)
    A = rs.standard_normal((rows, SK)).astype(np.float32)
    B = (rs.standard_normal((SK, SN)) * 1.5).astype(np.float32)
    alpha = 0.375 if transposed_b else 1.0
    R, lse, cross = _softmax_rows(ctx, A, SK, B, transposed_b, alpha)
    logits = alpha * (A.astype(np.float64) @ B.astype(np.float64))
    m = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - m)
    want = e / e.sum(axis=1, keepdims=True)
    lse_w, cross_w = (m + np.log(e.sum(axis=1, keepdims=True)))[:, 0], (want * logits).sum(axis=1)
    scale = np.abs(logits).max() + 1.0
    print("gemm_softmax_rows rows=%d raw n_iter=%d%s: R err / bound %.3g, lse %.3g, cross %.3g, row sums %.3g" % (
        rows, raw, " B^T" if transposed_b else "", (np.abs(R - want) / (2e-5 * np.abs(want) + 2e-6)).max(),
        np.abs(lse - lse_w).max() / (1e-5 * scale), np.abs(cross - cross_w).max() / (2e-5 * scale),
        np.abs(R.sum(axis=1) - 1.0).max() / 1e-5))
    npt.assert_allclose(R, want, rtol=2e-5, atol=2e-6)
    npt.assert_allclose(lse, lse_w, rtol=0, atol=1e-5 * scale)
    npt.assert_allclose(cross, cross_w, rtol=0, atol=2e-5 * scale)
    npt.assert_allclose(R.sum(axis=1), 1.0, rtol=1e-5)


@pytest.mark.parametrize("raw,write_r,bias", [(2, False, False), (2, True, False), (3, False, False), (3, True, False),
                                              (3, True, True), (2, False, True)])
def test_gemm_softmax_stats_through_the_buffer_alternation(ctx, cu, raw, write_r, bias):
    rows = softmax_rows_for("stats", "rebalanced", raw, cu)
    rs = np.random.RandomState(rows + SK + SN + (7 if bias else 0))
    lda = SK + 8
    A = (rs.standard_normal((rows, SK)) * 0.7).astype(np.float32)
    B = (rs.standard_normal((SK + 1, SN)) * 0.8).astype(np.float32)
    alpha = 1.1 if bias else 0.9
    got, lse, R = _softmax_stats(ctx, A, lda, B, alpha, write_r, bias)
    A64 = A.astype(np.float64)
    if bias:                                    # the same logits with a ones column IN the product
        A64 = np.concatenate([A64, np.ones((rows, 1))], axis=1)
    L = alpha * (A64 @ B.astype(np.float64)[:A64.shape[1]])
    m = L.max(axis=1, keepdims=True)
    e = np.exp(L - m)
    Rr = e / e.sum(axis=1, keepdims=True)
    Sr, lr = Rr.T @ A64, (m[:, 0] + np.log(e.sum(axis=1))).sum()
    bound = np.abs(Rr).T @ np.abs(A64)
    print("gemm_softmax_stats rows=%d raw n_iter=%d write_r=%d bias=%d: stats err / bound %.3g, lse %.3g of 2e-6%s" % (
        rows, raw, write_r, bias, (np.abs(got - Sr) / (3e-6 * bound + 1e-6)).max(), abs(lse - lr) / (2e-6 * abs(lr)),
        ", R err / bound %.3g" % (np.abs(R - Rr) / (2e-5 * np.abs(Rr) + 2e-7)).max() if write_r else ""))
    assert (np.abs(got - Sr) <= 3e-6 * bound + 1e-6).all(), np.abs(got - Sr).max()
    npt.assert_allclose(lse, lr, rtol=2e-6)
    if write_r:
        npt.assert_allclose(R, Rr, rtol=2e-5, atol=2e-7)


@pytest.mark.parametrize("raw", [2, 4])
def test_gemm_softmax_rows_exact_on_zero_logits(ctx, cu, raw):
    rows = softmax_rows_for("rows", "rebalanced", raw, cu)
    A = mr.small_ints((rows, SK), rows).astype(np.float32)
    R, lse, cross = _softmax_rows(ctx, A, SK, np.zeros((SK, SN), np.float32), False, 1.0)
    npt.assert_array_equal(R, np.full((rows, SN), 1.0 / 64, np.float32))
    npt.assert_array_equal(cross, np.zeros(rows, np.float32))
    npt.assert_allclose(lse, math.log(64.0), rtol=0, atol=1e-5)          # the parity test's bound at |logit| = 0


@pytest.mark.parametrize("raw,write_r", [(2, False), (2, True), (3, False), (3, True)])
def test_gemm_softmax_stats_exact_on_zero_logits(ctx, cu, raw, write_r):
    rows = softmax_rows_for("stats", "rebalanced", raw, cu)
    Ai = mr.small_ints((rows, SK), rows + 1)
    got, lse, R = _softmax_stats(ctx, Ai.astype(np.float32), SK, np.zeros((SK, SN), np.float32), 1.0, write_r)
    want = (Ai.sum(axis=0, dtype=np.int64) / 64.0).astype(np.float32)     # |sum| < 2^24: exact
    npt.assert_array_equal(got, np.broadcast_to(want, (SN, SK)))
    npt.assert_allclose(lse, rows * math.log(64.0), rtol=2e-6)
    if write_r:
        npt.assert_array_equal(R, np.full((rows, SN), 1.0 / 64, np.float32))


# ---- 3. bsc_weighted_outer ----------------------------------------------------------------------------------------

# name -> (K, D, E, symmetric, pad, KT, gy)
WO_CONFIGS = {
    "kt1_gy4": (32, 32, 32, False, (0, 0, 0), 1, 4),
    "kt2_gy2": (64, 16, 12, False, (0, 0, 0), 2, 2),
    "kt2_gy2_padded": (64, 16, 12, False, (4, 8, 12), 2, 2),
    "symmetric": (64, 16, 16, True, (0, 0, 0), 2, 1),
}
WO_CASES = [(name, iters) for name in ("kt1_gy4", "kt2_gy2", "symmetric") for iters in (2, 3)] + [("kt2_gy2_padded", 3)]


def wouter_rows(name, iters, cu):
    K, D, E, sym, _, KT, gy = WO_CONFIGS[name]
    N = mr.wouter_rows(iters, K, D, E, sym, cu)
    g = mr.wouter_grid(N, K, D, E, sym, cu)
    assert (g["iters"], g["KT"], g["gy"]) == (iters, KT, gy) and g["gx"] > 1, (N, cu, g)
    return N


@pytest.mark.parametrize("name,iters", WO_CASES)
def test_weighted_outer_exact_row_accounting(ctx, cu, name, iters):
    K, D, E, sym, pad, _, _ = WO_CONFIGS[name]
    N = wouter_rows(name, iters, cu)
    R, hot = mr.one_hot_rows(N, K, N + K)
    Xi = mr.small_ints((N, D), N + 1)
    Yi = Xi if sym else mr.small_ints((N, E), N + 2)
    got = wo_run(ctx, R, Xi.astype(np.float32), None if sym else Yi.astype(np.float32), scale=1.0, pad=pad)
    npt.assert_array_equal(got, mr.wouter_exact_reference(hot, Xi, Yi, K))


@pytest.mark.parametrize("name,iters", WO_CASES)
def test_weighted_outer_matches_float64_over_several_stages(ctx, cu, name, iters):
    K, D, E, sym, pad, _, _ = WO_CONFIGS[name]
    N = wouter_rows(name, iters, cu)
    rs = np.random.RandomState(N + K + D)
    X = rs.standard_normal((N, D)).astype(np.float32)
    if sym:                                 # test_wouter_gpu.test_symmetric_second_moment
        R = rs.dirichlet(np.ones(K), N).astype(np.float32)
        Y, scale = X, 0.5
    else:                                   # test_wouter_gpu.test_two_different_factors_and_padded_rows
        R = rs.standard_normal((N, K)).astype(np.float32)
        Y, scale = rs.standard_normal((N, E)).astype(np.float32), -2.0
    got = wo_run(ctx, R, X, None if sym else Y, scale=scale, pad=pad)
    want, bound = mr.wouter_reference(R, X, Y, scale)
    print("weighted_outer %s N=%d iters=%d: err / bound %.3g" % (name, N, iters,
                                                                 (np.abs(got - want) / (2e-5 * bound + 1e-30)).max()))
    assert (np.abs(got - want) <= 2e-5 * bound + (1e-30 if sym else 0.0)).all()
    if sym:
        npt.assert_array_equal(got, got.transpose(0, 2, 1))       # mirrored halves are the same bits
