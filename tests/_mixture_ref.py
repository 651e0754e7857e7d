"""Shared by tests/test_mixture_multi_tile_gpu.py and tests/test_mixture_multi_tile_cpu.py (numpy only: no device).

 * The host grid arithmetic of the mixture's three local-step routes, restated: bsc_mog_estep (csrc/bsc_mog.hip),
   bsc_gemm_softmax_rows / bsc_gemm_softmax_stats (csrc/bsc_rowsoftmax.hip) and bsc_weighted_outer (csrc/bsc_wouter.hip),
   and the row counts that reach a wanted number of tiles per wave (stages per workgroup).
 * The inputs of the exact-accounting cases and their int64 references.
 * `estep_standin`: the E-step's tile schedule (waves x n_iter, two alternating row buffers) in float64 numpy, with three
   injectable defects."""
import numpy as np

MT = 32                  # rows per tile: MT of csrc/bsc_mog.hip, RS_T of csrc/bsc_rowsoftmax.hip
WAVES = 4                # waves per workgroup of both (MOG_WAVES, RS_WAVES)
WO_TR = 64               # rows per stage of csrc/bsc_wouter.hip
EXP2_FLUSH = -150.0      # v_exp_f32(d) is exactly 0 for d below this (2^-149 is the smallest float32 denormal)


# ---- 0. the grids -----------------------------------------------------------------------------------------------

def cap(cu):
    """Rows of one sweep of the E-step / softmax grid: two waves per SIMD, 32-row tiles."""
    return 2 * 4 * cu * MT


def rows_rebalanced(it, cu):
    """One full tile and a ragged one of five rows beyond it - 1 full sweeps: the host re-balances the grid and the last
    iteration is nearly full."""
    return (it - 1) * cap(cu) + MT + 5


def rows_full_grid(it, cu):
    """Every wave slot of `it` sweeps used; the very last tile is ragged (5 rows)."""
    return it * cap(cu) - 27


def estep_grid(N, cu):
    """bsc_mog_estep: it = ceil(n_tiles / max_waves), waves = ceil(n_tiles / it), n_iter = it rounded up to even."""
    n_tiles = (N + MT - 1) // MT
    if n_tiles <= 0:
        return dict(n_tiles=0, it=0, n_iter=0, waves=0, n_blocks=1)
    max_waves = 2 * 4 * cu
    it = (n_tiles + max_waves - 1) // max_waves
    waves = (n_tiles + it - 1) // it
    return dict(n_tiles=n_tiles, it=it, n_iter=it + (it & 1), waves=waves, n_blocks=(waves + WAVES - 1) // WAVES)


def softmax_rows_grid(rows, cu):
    """bsc_gemm_softmax_rows: n_iter rounded up to a multiple of 3 (three row buffers rotate) BEFORE the grid is sized."""
    n_tiles = (rows + MT - 1) // MT
    max_waves = 2 * 4 * cu
    raw = (n_tiles + max_waves - 1) // max_waves
    n_iter = (raw + 2) // 3 * 3
    waves = (n_tiles + n_iter - 1) // n_iter if n_iter else 0
    return dict(n_tiles=n_tiles, raw=raw, n_iter=n_iter, waves=waves, n_blocks=(waves + WAVES - 1) // WAVES)


def softmax_stats_grid(rows, cu):
    """bsc_gemm_softmax_stats: n_iter rounded up to even (two row buffers alternate) BEFORE the grid is sized."""
    n_tiles = (rows + MT - 1) // MT
    max_waves = 2 * 4 * cu
    raw = (n_tiles + max_waves - 1) // max_waves if n_tiles > 0 else 0
    n_iter = raw + (raw & 1)
    waves = (n_tiles + n_iter - 1) // n_iter if n_iter else 0
    return dict(n_tiles=n_tiles, raw=raw, n_iter=n_iter, waves=waves, n_blocks=max(1, (waves + WAVES - 1) // WAVES))


def wouter_grid(N, K, D, E, sym, cu, wg_per_cu=2):
    """bsc_weighted_outer: KT component tiles, n_ct pair tiles split over gy columns of CT each, gx row workgroups that
    run `iters` stages of 64 rows."""
    P = D * (D + 1) // 2 if sym else D * E
    KT = (K + 31) // 32
    n_ct = (P + 31) // 32
    max_ct = 5 if KT == 2 else 8
    gy = (n_ct + max_ct - 1) // max_ct
    CT = (n_ct + gy - 1) // gy
    stages = (N + WO_TR - 1) // WO_TR
    gx0 = max(1, wg_per_cu * cu // gy)
    gx = min(gx0, max(stages, 1))
    iters = (stages + gx - 1) // gx
    if stages > 0:
        gx = (stages + iters - 1) // iters
    return dict(KT=KT, n_ct=n_ct, gy=gy, CT=CT, stages=stages, gx0=gx0, gx=gx, iters=iters)


def wouter_rows(iters, K, D, E, sym, cu, wg_per_cu=2):
    """iters - 1 sweeps of the row workgroups, one full stage and five rows."""
    gx0 = wouter_grid(1, K, D, E, sym, cu, wg_per_cu)["gx0"]
    return ((iters - 1) * gx0 + 1) * WO_TR + 5


# ---- 1. the E-step's inputs ---------------------------------------------------------------------------------------

def estep_exact_data(N, K, D):
    """Separated clusters, integer data, labels and offsets pseudo-random in the row: centres[k, k % D] = 24 (1 + k // D),
    unit precisions, offsets in [-2, 2], label(n) = (n + h[n // 32]) % K -- 32 distinct components in every tile (K > 32).
    -> X, Wmat, c, labels, want (int64 [K, 1 + 2 D])."""
    assert K > MT
    rs = np.random.RandomState(1000003 * K + 101 * D + N % 9973)
    k = np.arange(K)
    centres = np.zeros((K, D))
    centres[k, k % D] = 24.0 * (1 + k // D)
    n = np.arange(N)
    h = rs.randint(K, size=(N + MT - 1) // MT)
    labels = (n + h[n // MT]) % K
    offs = rs.randint(-2, 3, size=(N, D))
    Xi = centres[labels].astype(np.int64) + offs
    X = Xi.astype(np.float32)
    Wmat = np.concatenate([centres, -0.5 * np.ones((K, D))], axis=1).astype(np.float32)
    c = (-0.5 * (centres ** 2).sum(1)).astype(np.float32)
    want = np.zeros((K, 1 + 2 * D), np.int64)
    np.add.at(want, labels, np.concatenate([np.ones((N, 1), np.int64), Xi, Xi * Xi], axis=1))
    return X, Wmat, c, labels, want


def estep_overlap_data(N, D, K):
    """tests/test_mog_gpu.py::test_estep_matches_oracle's data: overlapping clusters."""
    rs = np.random.RandomState(N + D + K)
    centres = rs.standard_normal((K, D)) * 3
    X = (centres[rs.randint(K, size=N)] + rs.standard_normal((N, D))).astype(np.float32)
    T = rs.uniform(0.5, 2.0, (K, D))
    Wmat = np.concatenate([T * centres, -0.5 * T], axis=1).astype(np.float32)
    c = (rs.standard_normal(K) - 0.5 * (T * centres ** 2).sum(1)).astype(np.float32)
    return X, Wmat, c


def estep_scale(X):
    """The scale of test_estep_matches_oracle's bound 2e-5 * scale + 1e-9, per statistic column."""
    X64 = X.astype(np.float64)
    return np.concatenate([[max(X.shape[0], 1)], np.abs(X64).sum(0) + 1e-9, (X64 ** 2).sum(0) + 1e-9])


def log2_margin_f32(X, Wmat, c, labels):
    """Smallest (l_own - l_best other) log2 e over the rows, the logits in float32 as the kernel forms them (natural
    units, float32 products and sums): what v_exp_f32 is given for the best of the other components."""
    F = np.concatenate([X, X * X], axis=1).astype(np.float32)
    L = F @ Wmat.T + c[None, :]
    assert L.dtype == np.float32
    rows = np.arange(X.shape[0])
    own = L[rows, labels].copy()
    L[rows, labels] = -np.inf
    return float((own - L.max(axis=1)).min() * np.float32(1.4426950408889634))


def estep_lse_f32(X, Wmat, c, labels, prescaled):
    """sum_n lse_n on one-hot data (every other term of the softmax is exactly 0: lse_n is the own component's logit) from
    a float32 fma chain as mog_estep_kernel runs it: the bias as the accumulator's start, then k-step s adding x_s W[s]
    and x_s^2 W[D + s] with one rounding each; float64 sum over the rows.
    prescaled: W and c times log2 e, each rounded to float32, and ln 2 times the result -- how the kernels formed the
    logits before they were changed to natural units (prescaled = False)."""
    scale = np.float32(1.4426950408889634) if prescaled else np.float32(1.0)
    D = X.shape[1]
    rows = np.arange(X.shape[0])
    W2, acc = (Wmat * scale)[labels], (c * scale)[labels]
    assert W2.dtype == np.float32 and acc.dtype == np.float32
    F = np.concatenate([X, X * X], axis=1)
    for s in range(D):
        for j in (s, D + s):
            acc = (acc.astype(np.float64) + F[rows, j].astype(np.float64) * W2[rows, j].astype(np.float64)).astype(np.float32)
    return float((0.6931471805599453 if prescaled else 1.0) * acc.astype(np.float64).sum())


# ---- 2. / 3. the exact inputs of the softmax passes and of the weighted outer product -------------------------------

def small_ints(shape, seed, lo=-3, hi=3):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape)


def one_hot_rows(N, K, seed):
    hot = np.random.RandomState(seed).randint(K, size=N)
    R = np.zeros((N, K), np.float32)
    R[np.arange(N), hot] = 1.0
    return R, hot


def wouter_exact_reference(hot, Xi, Yi, K):
    """sum_n 1[hot_n = k] X[n, d] Y[n, e] in int64 (rows sorted by their hot column, then one sum per run)."""
    order = np.argsort(hot, kind="stable")
    starts = np.searchsorted(hot[order], np.arange(K))
    assert (np.diff(np.append(starts, len(hot))) > 0).all()      # every component owns rows (reduceat needs that)
    prod = Xi.astype(np.int64)[order][:, :, None] * Yi.astype(np.int64)[order][:, None, :]
    return np.add.reduceat(prod, starts, axis=0)


def wouter_reference(R, X, Y, scale=1.0, chunk=4096):
    """tests/test_wouter_gpu.py's reference() -- float64 sum_n R[n,k] X[n,d] Y[n,e] and the sum of the terms' magnitudes
    -- as chunked matrix products: its three-operand einsum takes 14 s at the largest shape used here."""
    R, X, Y = (a.astype(np.float64) for a in (R, X, Y))
    K, D, E = R.shape[1], X.shape[1], Y.shape[1]
    want, bound = np.zeros((K, D * E)), np.zeros((K, D * E))
    for i in range(0, R.shape[0], chunk):
        r, z = R[i:i + chunk], (X[i:i + chunk, :, None] * Y[i:i + chunk, None, :]).reshape(-1, D * E)
        want += r.T @ z
        bound += np.abs(r).T @ np.abs(z)
    return scale * want.reshape(K, D, E), abs(scale) * bound.reshape(K, D, E)


# ---- 4. a stand-in of the E-step's schedule -------------------------------------------------------------------------

DEFECTS = ("skip_last_tile", "previous_buffer", "ragged_padding")


def estep_standin(X, Wmat, c, cu, defect=None, wave=1):
    """mog_estep_kernel's schedule in float64: wave w of n_blocks * 4 runs n_iter (even) trips; trip `it` contracts row
    buffer it & 1, which holds tile w + it * stride (rows past N read as zero and are masked), after prefetching tile
    w + (it + 1) * stride into the other buffer.  exp2 flushes to zero below 2^-149 as v_exp_f32 does, so one-hot
    responsibilities are exactly one-hot.
    defect (in wave `wave` only, except the last):
      skip_last_tile   the trip of the wave's last non-empty tile is not run;
      previous_buffer  the wave's second trip contracts the rows of its first again (tile w twice, tile w + stride never);
      ragged_padding   the ragged tile's padding rows (zeros) are counted as rows.
    -> stats [K, 1 + 2 D], lse."""
    assert defect in (None,) + DEFECTS
    N, D = X.shape
    K = Wmat.shape[0]
    g = estep_grid(N, cu)
    stride = g["n_blocks"] * WAVES
    log2e, ln2 = 1.4426950408889634, 0.6931471805599453
    W2, c2 = Wmat.astype(np.float64) * log2e, c.astype(np.float64) * log2e
    X64 = X.astype(np.float64)

    def load(tile):
        rows = np.zeros((MT, D))
        lo = tile * MT
        if lo < N:
            rows[:min(MT, N - lo)] = X64[lo:lo + MT]
        return tile, rows

    stats, lse = np.zeros((K, 1 + 2 * D)), 0.0
    for w in range(stride):
        last_real = max((t for t in range(w, g["n_tiles"], stride)), default=-1)
        buf = [load(w), None]
        tile = w
        for it in range(g["n_iter"]):
            buf[1 - (it & 1)] = load(tile + stride)
            held, x = buf[it & 1]
            if defect == "previous_buffer" and w == wave and it == 1:
                held, x = prev
            prev = (held, x)
            tile += stride
            if defect == "skip_last_tile" and w == wave and held == last_real:
                continue
            valid = held * MT + np.arange(MT) < N
            if defect == "ragged_padding" and 0 < N - held * MT < MT:
                valid[:] = True
            if not valid.any():
                continue
            F = np.concatenate([x, x * x], axis=1)
            L = F @ W2.T + c2[None, :]
            m = L.max(axis=1, keepdims=True)
            d = L - m
            e = np.where(d < EXP2_FLUSH, 0.0, np.exp2(d))
            s = e.sum(axis=1, keepdims=True)
            r = np.where(valid[:, None], e / s, 0.0)
            lse += float((ln2 * (m[:, 0] + np.log2(s[:, 0])))[valid].sum())
            stats[:, 0] += r.sum(axis=0)
            stats[:, 1:] += r.T @ F
    return stats, lse
