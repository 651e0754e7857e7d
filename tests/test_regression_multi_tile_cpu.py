"""CPU companion of tests/test_regression_multi_tile_gpu.py.  No test here touches a device.

 * The grid arithmetic that module restates, at 256 CUs (an MI355X): its batches come out at the tiles-per-wave they
   are built for.
 * The tolerances it borrows were derived per row and per term, not per batch size: a plain float32 evaluation of each
   reference on the CPU (float32 dots, transcendentals and per-row terms; sums over rows as the device takes them, in
   float32 for G and in float64 for ell and lpd_sum) stays inside them at the largest batch that module uses at 256
   CUs, one shape per entry point -- tests/test_softmax_cpu.py's check at the new row count.  A bound that a float32
   evaluation misses would be wrong, not the device."""
import math

import numpy as np
import pytest
from scipy.special import gammaln

import _glm_ref as glm
import _predict_ref as pref
import _softmax_ref as sref
import test_regression_multi_tile_gpu as mt

f32 = np.float32
B_BIG = 65557


@pytest.mark.parametrize("rows,n_iter,B,n_tiles", [(16, 2, 32789, 2050), (16, 3, 65557, 4098), (8, 3, 32781, 4098),
                                                   (8, 4, 49165, 6146), (8, 5, 65549, 8194)])
def test_batches_reach_their_tiles_per_wave_at_256_cus(rows, n_iter, B, n_tiles):
    assert mt.rows_for(n_iter, rows, 256) == B == mt.batch(256, n_iter, rows) == mt.batch(256, n_iter, rows, 8)
    for wpb in (4, 8):
        g = mt.grid(B, rows, 256, wpb)
        assert g["n_iter"] == n_iter and g["n_tiles"] == n_tiles
        assert g["waves"] <= 2048 and g["waves"] * n_iter >= n_tiles > g["waves"] * (n_iter - 1)
        assert g["n_blocks"] * wpb >= g["waves"] > (g["n_blocks"] - 1) * wpb
    # one row fewer than a full sweep more, and the loop is one trip shorter
    assert mt.grid((n_iter - 1) * 2048 * rows, rows, 256)["n_iter"] == n_iter - 1
    assert mt.grid((n_iter - 1) * 2048 * rows + 1, rows, 256)["n_iter"] == n_iter


def test_the_grid_at_the_flagship_size_and_at_the_edges():
    assert mt.grid(1 << 20, 16, 256)["n_iter"] == 32 and mt.grid(1000000, 16, 256)["n_iter"] == 31
    assert mt.grid(65557, 16, 256) == dict(n_tiles=4098, n_iter=3, waves=1366, n_blocks=342)
    assert mt.grid(65557, 16, 256, 8)["n_blocks"] == 171
    assert mt.grid(0, 16, 256) == dict(n_tiles=0, n_iter=0, waves=0, n_blocks=1)
    assert mt.grid(20000, 16, 256)["n_iter"] == 1 and mt.grid(20000, 8, 256)["n_iter"] == 2     # the older tests' largest
    rows = mt.probe_rows(65557)
    assert np.array_equal(np.unique(rows // 16), np.arange(4098)) and rows[-1] == 65556


def test_float32_glm_pass_stays_inside_the_bounds():
    X, y, W = mt.glm_t._inputs("logistic", B_BIG, 256, 8, 3)
    L = (X @ W.T).astype(f32)
    e = np.exp(-np.abs(L), dtype=f32)
    A = (np.maximum(L, f32(0)) + np.log1p(e, dtype=f32)).astype(f32)
    dA = (np.where(L >= 0, f32(1), e) / (f32(1) + e)).astype(f32)
    ell = (y[:, None] * L - A).astype(f32).sum(axis=0, dtype=np.float64)
    G = ((y[:, None] - dA).astype(f32).T @ X).astype(f32)
    ell_r, G_r = glm.glm_data_pass("logistic", X, y, W)
    L64 = X.astype(np.float64) @ W.astype(np.float64).T
    A64, _ = glm.log_partition("logistic", L64)
    bound = (np.abs(y.astype(np.float64)[:, None] * L64) + A64 + 1.0).sum(axis=0)
    assert (np.abs(ell - ell_r) <= 2e-5 * bound).all()
    assert (np.abs(G - G_r) <= 1e-4 * np.abs(G_r) + 1e-4 * np.abs(G_r).max()).all()


def test_float32_predict_pass_stays_inside_the_bounds():
    S = 17
    X, y, W, _ = mt.predict_t._inputs("poisson", B_BIG, 256, S, 3)
    L = (X @ W.T).astype(f32)
    mu = np.exp(L, dtype=f32)
    mean = (mu.sum(axis=1, dtype=f32) / f32(S)).astype(f32)
    var = ((mu.sum(axis=1, dtype=f32) + ((mu - mean[:, None]) ** 2).sum(axis=1, dtype=f32)) / f32(S)).astype(f32)
    lp = (y[:, None] * L - mu).astype(f32)
    mx = lp.max(axis=1, keepdims=True)
    lpd = (mx[:, 0] + np.log(np.exp(lp - mx, dtype=f32).sum(axis=1, dtype=f32), dtype=f32) - f32(math.log(S))
           - gammaln(y.astype(np.float64) + 1.0).astype(f32)).astype(f32)
    want, bnd = pref.predict("poisson", X, W, None, y), pref.bounds("poisson", X, W, None, y)
    got = dict(mean=mean, var=var, lpd=lpd, lpd_sum=lpd.sum(dtype=np.float64))
    for k in got:
        assert np.max(np.abs(got[k] - want[k]) / bnd[k]) <= 1.0, k


def _softmax_f32(X, y, W):
    """tests/test_softmax_cpu.py's float32 evaluation."""
    B, S = X.shape[0], W.shape[0]
    L = np.einsum("nd,skd->nsk", X, W).astype(f32)
    m = L.max(axis=2, keepdims=True)
    e = np.exp(L - m, dtype=f32)
    s = e.sum(axis=2, keepdims=True, dtype=f32)
    p = (e / s).astype(f32)
    lp = (L[np.arange(B), :, y] - (m[:, :, 0] + np.log(s[:, :, 0], dtype=f32))).astype(f32)
    mx = lp.max(axis=1, keepdims=True)
    lpd = (mx[:, 0] + np.log(np.exp(lp - mx, dtype=f32).sum(axis=1, dtype=f32), dtype=f32) - f32(math.log(S))).astype(f32)
    return p, lp, lpd


def test_float32_softmax_passes_stay_inside_the_bounds():
    K, S = 5, 4
    X, y, W = mt.softmax_t._inputs(B_BIG, 256, K, S, 5)
    p, lp, lpd = _softmax_f32(X, y, W)
    r, b = sref.predict(X, W, y), sref.predict_bounds(X, W, y)
    assert (np.abs(p.mean(axis=1, dtype=f32) - r["prob"]) <= b["prob"]).all()
    assert (np.abs(lpd - r["lpd"]) <= b["lpd"]).all()
    assert abs(lpd.sum(dtype=np.float64) - r["lpd_sum"]) <= b["lpd_sum"]
    ell_r, G_r = sref.softmax_data_pass(X, y, W)
    assert (np.abs(lp.sum(axis=0, dtype=np.float64) - ell_r) <= 2e-5 * sref.ell_bound(X, y, W)).all()
    R = -p
    R[np.arange(B_BIG), :, y] += f32(1)
    G = np.einsum("nsk,nd->skd", R, X, optimize=True).astype(f32)
    assert (np.abs(G - G_r) <= 1e-4 * np.abs(G_r) + 1e-4 * np.abs(G_r).max()).all()
