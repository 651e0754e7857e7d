"""CPU companion of tests/test_mixture_multi_tile_gpu.py.  No test here touches a device.

 * The three shape tables at 256 CUs (an MI355X) with the n_iter / iters each row reaches, from the host grids restated
   in tests/_mixture_ref.py.
 * The preconditions of every exact construction of the GPU module: the float32 log2-logit margin that makes the
   responsibilities exactly one-hot, x^2 < 2^16 (two bf16 terms hold it), and every float32 partial sum an integer
   (a multiple of 1/64 for the softmax statistics) below 2^24.
 * _mixture_ref.estep_standin, the E-step's tile schedule in float64, with one defect at a time:
     - each defect FAILS the exact comparison of the GPU module's 1(a);
     - the buffer defect (one wave contracts the rows of its first trip twice and the second trip's never) moves the
       statistics by one tile's worth whatever N is, while the borrowed parity bounds grow with N.  Measured with the
       stand-in on the overlapping data of 1(b): at N = 8 229 the move is 122 x the bound 2e-5 scale, so at the 10M rows of
       tests/test_full_size_gpu.py and tests/test_oracle_c.py -- the only f32 tests that ran several tiles per wave before
       -- it is 0.10 x the bound, sum R = N holds exactly and lse moves by 0.05 of its rtol: those tests stay green.
       That is why the exact cases exist.  At the GPU module's own row counts (65 573 .. 262 181) a whole mis-buffered tile
       is 4 to 15 x the parity bound, so there 1(b) would see it as well; a defect of a few rows would still pass it.
 * The float32 evaluation of the logit chain that shows why the E-step forms its logits in natural units: with
   coefficients scaled by log2 e beforehand, lse on the exact data misses rtol 2e-6 by up to 43 x."""
import numpy as np
import numpy.testing as npt
import pytest

import _mixture_ref as mr
from oracle import svi

CU = 256


# ---- the shape tables at 256 CUs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("it,N,n_iter,n_tiles,waves", [(2, 65573, 2, 2050, 1025), (3, 131109, 4, 4098, 1366),
                                                       (4, 196645, 4, 6146, 1537), (5, 262181, 6, 8194, 1639)])
def test_estep_rows_reach_their_tiles_per_wave(it, N, n_iter, n_tiles, waves):
    assert mr.rows_rebalanced(it, CU) == N
    g = mr.estep_grid(N, CU)
    assert g == dict(n_tiles=n_tiles, it=it, n_iter=n_iter, waves=waves, n_blocks=(waves + 3) // 4)
    assert g["waves"] * it >= n_tiles > g["waves"] * (it - 1) and g["waves"] <= 2048
    # one row fewer than a full sweep more, and the loop is one trip shorter
    assert mr.estep_grid((it - 1) * mr.cap(CU), CU)["it"] == it - 1
    assert mr.estep_grid((it - 1) * mr.cap(CU) + 1, CU)["it"] == it
    # the full-grid form: every wave slot used, the last tile ragged
    F = mr.rows_full_grid(it, CU)
    f = mr.estep_grid(F, CU)
    assert (f["it"], f["waves"], f["n_tiles"], F % 32) == (it, 2048, 2048 * it, 5)


def test_estep_grid_at_the_older_tests_sizes():
    assert mr.cap(CU) == 65536 and mr.rows_full_grid(2, CU) == 131045
    assert mr.estep_grid(40000, CU)["it"] == 1 and mr.estep_grid(40000, CU)["n_iter"] == 2    # the second tile is empty
    assert mr.estep_grid(300000, CU)["it"] == 5 and mr.estep_grid(10_000_000, CU)["it"] == 153
    assert mr.estep_grid(0, CU) == dict(n_tiles=0, it=0, n_iter=0, waves=0, n_blocks=1)


@pytest.mark.parametrize("raw,rows,rows_n_iter,stats_n_iter", [(2, 65573, 3, 2), (3, 131109, 3, 4), (4, 196645, 6, 4)])
def test_softmax_rows_reach_their_rotations(raw, rows, rows_n_iter, stats_n_iter):
    assert mr.rows_rebalanced(raw, CU) == rows
    r, s = mr.softmax_rows_grid(rows, CU), mr.softmax_stats_grid(rows, CU)
    assert (r["raw"], r["n_iter"]) == (raw, rows_n_iter) and (s["raw"], s["n_iter"]) == (raw, stats_n_iter)
    for g in (r, s):              # the grid is sized for the ROUNDED trip count: every tile has a slot, none twice
        assert g["waves"] * g["n_iter"] >= g["n_tiles"] > (g["waves"] - 1) * g["n_iter"]
        assert g["n_blocks"] * 4 >= g["waves"] > (g["n_blocks"] - 1) * 4
    assert mr.softmax_rows_grid(70001, CU)["raw"] == 2 == mr.softmax_stats_grid(70001, CU)["raw"]   # the older largest
    f = mr.softmax_rows_grid(mr.rows_full_grid(2, CU), CU)
    assert (f["raw"], f["n_iter"], f["n_tiles"]) == (2, 3, 4096)


@pytest.mark.parametrize("K,D,E,sym,KT,gy,CT,gx0,rows2,rows3", [
    (32, 32, 32, False, 1, 4, 8, 128, 8261, 16453), (64, 16, 12, False, 2, 2, 3, 256, 16453, 32837),
    (64, 16, 16, True, 2, 1, 5, 512, 32837, 65605)])
def test_weighted_outer_rows_reach_their_stages(K, D, E, sym, KT, gy, CT, gx0, rows2, rows3):
    for iters, N in ((2, rows2), (3, rows3)):
        assert mr.wouter_rows(iters, K, D, E, sym, CU) == N
        g = mr.wouter_grid(N, K, D, E, sym, CU)
        assert (g["KT"], g["gy"], g["CT"], g["gx0"], g["iters"]) == (KT, gy, CT, gx0, iters)
        assert g["gx"] * iters >= g["stages"] > g["gx"] * (iters - 1) and g["gx"] <= gx0
    assert mr.wouter_grid(70000, 64, 16, 16, True, CU)["iters"] == 3           # the one older case with iters > 1
    assert mr.wouter_grid(2000, 12, 32, 32, False, CU)["iters"] == 1


# ---- the preconditions of the exact constructions -----------------------------------------------------------------

@pytest.mark.parametrize("N,K,D", [(65573, 64, 16), (131109, 64, 16), (262181, 64, 16), (131045, 64, 16), (65573, 64, 12),
                                   (131109, 64, 12), (262181, 64, 12), (65573, 33, 5), (131109, 33, 5), (262181, 33, 5)])
def test_exact_estep_construction_is_exact_in_float32(N, K, D):
    X, Wmat, c, labels, want = mr.estep_exact_data(N, K, D)
    # one-hot: exp2 of every other component's distance to the row maximum is exactly 0
    margin = mr.log2_margin_f32(X, Wmat, c, labels)
    assert margin >= 346 > -mr.EXP2_FLUSH, margin
    # x^2 < 2^16: exact in two bf16 terms (the split route's backward operand), x itself in one
    assert np.abs(X).max() <= 170 and float(np.abs(X).max()) ** 2 < 2 ** 16
    # a tile holds 32 distinct components, so a wave adds at most one row per component and trip, a workgroup 4 n_iter
    tiles = labels[:N // 32 * 32].reshape(-1, 32)
    assert (np.sort(tiles, axis=1)[:, 1:] != np.sort(tiles, axis=1)[:, :-1]).all()
    n_iter = mr.estep_grid(N, CU)["n_iter"]
    assert 4 * n_iter * float(np.abs(X).max()) ** 2 < 2 ** 24
    # the reference: int64 sums per label, and they are what float64 holds exactly
    assert want.dtype == np.int64 and want[:, 0].sum() == N and np.abs(want).max() < 2 ** 53
    onehot = np.zeros((N, K))
    onehot[np.arange(N), labels] = 1.0
    X64 = X.astype(np.float64)
    npt.assert_array_equal(want, onehot.T @ np.concatenate([np.ones((N, 1)), X64, X64 * X64], axis=1))
    # the data are no function of the row modulo the grid: consecutive sweeps differ in every tile
    sweep = mr.estep_grid(N, CU)["n_blocks"] * 4 * 32
    m = min(sweep, N - sweep)
    assert (X[:m] != X[sweep:sweep + m]).any(axis=1).mean() > 0.99


@pytest.mark.parametrize("rows", [65573, 131109, 196645])
def test_exact_softmax_construction_is_exact_in_float32(rows):
    for seed in (rows, rows + 1):
        A = mr.small_ints((rows, 40), seed)
        assert A.min() == -3 and A.max() == 3
        # statistics: multiples of 1/64 whose numerators stay below 2^24 at every partial sum
        assert 3 * rows < 2 ** 24
        want = (A.sum(axis=0, dtype=np.int64) / 64.0).astype(np.float32)
        npt.assert_array_equal(want.astype(np.float64) * 64, A.sum(axis=0))
    assert np.float32(1.0) / np.float32(64.0) == np.float32(2.0 ** -6)


@pytest.mark.parametrize("K,D,E,sym,N", [(32, 32, 32, False, 16453), (64, 16, 12, False, 32837), (64, 16, 16, True, 65605)])
def test_exact_weighted_outer_construction_and_the_fast_reference(K, D, E, sym, N):
    R, hot = mr.one_hot_rows(N, K, N + K)
    Xi = mr.small_ints((N, D), N + 1)
    Yi = Xi if sym else mr.small_ints((N, E), N + 2)
    assert 9 * N < 2 ** 24                                   # every partial sum and the float32 result are integers
    want = mr.wouter_exact_reference(hot, Xi, Yi, K)
    assert want.dtype == np.int64 and want.shape == (K, D, E)
    fast, bound = mr.wouter_reference(R, Xi.astype(np.float32), Yi.astype(np.float32))
    npt.assert_array_equal(fast, want)
    assert (np.abs(want) <= bound).all()
    # the fast float64 reference IS test_wouter_gpu.reference (its einsum, on a batch it handles quickly)
    rs = np.random.RandomState(N)
    n = 700
    Rr, Xr, Yr = (rs.standard_normal((n, m)).astype(np.float32) for m in (K, D, E))
    w_e = -2.0 * np.einsum("nk,nd,ne->kde", *(a.astype(np.float64) for a in (Rr, Xr, Yr)))
    b_e = 2.0 * np.einsum("nk,nd,ne->kde", *(np.abs(a.astype(np.float64)) for a in (Rr, Xr, Yr)))
    w_f, b_f = mr.wouter_reference(Rr, Xr, Yr, -2.0, chunk=256)
    npt.assert_allclose(w_f, w_e, rtol=0, atol=1e-12 * b_e.max())
    npt.assert_allclose(b_f, b_e, rtol=1e-12)


@pytest.mark.parametrize("N,K,D,ratio", [(65573, 64, 16, 0.17), (65573, 64, 12, 16.4), (65573, 33, 5, 42.9)])
def test_logits_in_natural_units_meet_the_lse_tolerance_on_the_exact_data(N, K, D, ratio):
    """Why mog_estep_kernel forms its logits from W and c as given and multiplies (l - m) by log2 e afterwards.  With the
    coefficients scaled by log2 e and rounded first, the float32 chain alone -- no tiles, no waves, no buffers -- is
    `ratio` x the rtol of 2e-6 away from the float64 oracle (what the device returned then: 0.17, 16.4, 42.9); in natural
    units every product and partial sum of these data is a half-integer below 2^24 and the chain is exact."""
    X, Wmat, c, labels, _ = mr.estep_exact_data(N, K, D)
    _, lse_ref = svi.mog_local_step(X, Wmat, c)
    got = abs(mr.estep_lse_f32(X, Wmat, c, labels, prescaled=True) - lse_ref) / (2e-6 * abs(lse_ref))
    assert abs(got - ratio) <= 0.03 * ratio, got
    terms = float(np.abs(X).max()) * float(np.abs(Wmat[:, :D]).max()) * 1.4426950408889634
    assert abs(got * 2e-6 * lse_ref / N) <= 3 * 2.0 ** -24 * terms          # per row: three roundings of one term's size
    assert mr.estep_lse_f32(X, Wmat, c, labels, prescaled=False) == lse_ref


# ---- the stand-in: what the exact cases see and the parity cases do not -------------------------------------------

SMALL_CU = 16                 # the schedule's arithmetic is the same at any CU count: 128 waves instead of 2048


@pytest.mark.parametrize("it", [2, 3, 5])
def test_standin_is_exact_and_every_defect_breaks_exact_accounting(it):
    N = mr.rows_rebalanced(it, SMALL_CU)
    assert mr.estep_grid(N, SMALL_CU)["n_iter"] == it + (it & 1)
    X, Wmat, c, labels, want = mr.estep_exact_data(N, 64, 16)
    clean, lse = mr.estep_standin(X, Wmat, c, SMALL_CU)
    npt.assert_array_equal(clean, want)
    npt.assert_allclose(lse, svi.mog_local_step(X, Wmat, c)[1], rtol=1e-12)
    for defect in mr.DEFECTS:
        bad, _ = mr.estep_standin(X, Wmat, c, SMALL_CU, defect=defect)
        assert not np.array_equal(bad, want), defect
        if defect == "previous_buffer":         # rows are neither lost nor gained: conservation sums cannot see it
            assert bad[:, 0].sum() == N


def test_buffer_defect_passes_the_borrowed_parity_bounds_at_the_older_tests_size():
    N, N_OLD = mr.rows_rebalanced(3, SMALL_CU), 10_000_000
    X, Wmat, c = mr.estep_overlap_data(N, 16, 64)
    want, lse_ref = svi.mog_local_step(X, Wmat, c)
    scale = mr.estep_scale(X)
    clean, lse = mr.estep_standin(X, Wmat, c, SMALL_CU)
    assert (np.abs(clean - want) <= 1e-9 * scale[None, :]).all() and abs(lse - lse_ref) <= 1e-12 * abs(lse_ref)
    bad, lse_bad = mr.estep_standin(X, Wmat, c, SMALL_CU, defect="previous_buffer")
    # what one mis-buffered tile moves does not depend on N; the bounds are sums over the rows and grow with it
    moved = np.abs(bad - want) / (2e-5 * scale[None, :] + 1e-9)
    assert moved.max() > 1.0                                        # at this N the parity bound would see it ...
    grow = N_OLD / N
    assert moved.max() / grow < 1.0                                 # ... at 10M rows it is inside the bound (0.10 of it)
    assert abs(bad[:, 0].sum() - N) <= 1e-6 * N                     # sum R = N: holds at any N
    assert abs(lse_bad - lse_ref) / grow <= 2e-6 * abs(lse_ref)
    # and the exact construction at the same shape sees it
    Xe, We, ce, _, want_e = mr.estep_exact_data(N, 64, 16)
    assert not np.array_equal(mr.estep_standin(Xe, We, ce, SMALL_CU, defect="previous_buffer")[0], want_e)
