"""float64 (and float32-in / float64-inside) kernels of csrc/bsc_tensor.hip, csrc/bsc_gemm.hip, csrc/bsc_fused.hip and
csrc/bsc_stats.hip through the C ABI, against numpy / scipy in float64.

Tolerances are float64 bounds wherever the kernel computes in float64:
* Cholesky (bsc_logdet_spd, bsc_inverse_spd): the matrices are built with a chosen spectrum (condition number kappa),
  and the backward-stable Cholesky gives |d logdet| <= ~n kappa u and ||d inv|| <= ~n kappa u ||inv|| (u = 2^-53);
  the bounds below are 8 n kappa u, plus one float32 rounding of the result where the output is float32.
* element-wise float64 ops: device libm to a few ulp, n-ary sums / products in a fixed order (a few ulp per operand).
* the naive float64 GEMM: a k-ordered fma chain, |error| <= K u sum_k |a_k b_k| (times 2 for the reference's own).
* special functions: bsc_digamma_f64 as in tests/test_special_host.py (1e-13 relative + 2e-15 absolute), HIP's
  lgamma to 1e-13 relative + 2e-14 absolute; the Dirichlet entries take and return float32, so their outputs are
  compared at two float32 roundings (the reference's and the kernel's) of the float64 scipy value.
Only positive finite arguments reach the special functions here: the others are tested on the host."""
import builtins
import ctypes

import numpy as np
import pytest
import torch
from scipy import special

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
F32_ULP = 2.0 ** -23
OPS = {"add": 0, "mul": 1, "log": 2, "exp": 3, "pow": 4, "abs_": 5, "copy": 6, "gammaln": 7, "digamma": 8}


def _i64(v):
    v = list(v)
    return (ctypes.c_int64 * builtins.max(len(v), 1))(*v)


def _spd(rs, n, kappa):
    """Symmetric positive definite, eigenvalues log-spaced over [1, kappa]; exactly symmetric in float64."""
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    lam = np.logspace(0.0, np.log10(kappa), n) if n > 1 else np.array([kappa])
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T)


def _padded(ctx, mats, dtype, transposed):
    """The batch [b, n, n] inside a NaN-filled buffer: rows ld = n + 3 apart, matrices a stride apart that is not
    n * ld; transposed: the same matrices read with (s_r, s_c) = (1, ld).  Returns (tensor, s_b, s_r, s_c)."""
    b, n, _ = mats.shape
    ld, sb = n + 3, (n + 3) * (n + 1) + 5
    buf = np.full(b * sb, np.nan, dtype)
    for i in range(b):
        block = mats[i].T if transposed else mats[i]
        view = buf[i * sb:i * sb + n * ld].reshape(n, ld)
        view[:, :n] = block
    s_r, s_c = (1, ld) if transposed else (ld, 1)
    return ctx.to_device(buf), sb, s_r, s_c


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n,batch", [(1, 70), (2, 3), (7, 70), (64, 3), (255, 1), (256, 3)])
def test_logdet_and_inverse_spd_against_numpy(ctx, dtype, n, batch):
    rs = np.random.RandomState(n * 1000 + batch)
    # (float32 input: kappa <= 1e3, so that rounding the entries, ~n 2^-24 kappa of the smallest eigenvalue, keeps
    # the matrix positive definite)
    kappas = [10.0 ** rs.uniform(0, 6 if dtype == np.float64 else 3) for _ in range(batch)]
    mats = np.stack([_spd(rs, n, k) for k in kappas]).astype(dtype)
    ref = mats.astype(np.float64)                          # the matrices the kernel receives
    want_ld = np.linalg.slogdet(ref)[1]
    want_inv = np.linalg.inv(ref)
    code = 1 if dtype == np.float64 else 0
    out_rounding = 0.0 if dtype == np.float64 else F32_ULP
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    for transposed in (False, True):
        A, sb, sr, sc = _padded(ctx, mats, dtype, transposed)
        ld = torch.full((batch,), float("nan"), dtype=tdt, device=ctx.device)
        ctx.call("bsc_logdet_spd", code, batch, n, A, sb, sr, sc, ld)
        inv = torch.full((batch, n, n), float("nan"), dtype=tdt, device=ctx.device)
        ld2 = torch.full((batch,), float("nan"), dtype=tdt, device=ctx.device)
        ctx.call("bsc_inverse_spd", code, batch, n, A, sb, sr, sc, inv, ld2)
        ctx.sync()
        got_ld, got_inv, got_ld2 = ld.cpu().numpy(), inv.cpu().numpy(), ld2.cpu().numpy()
        for i, kappa in enumerate(kappas):
            kappa = np.linalg.cond(ref[i])                   # (of the matrix as rounded to the input dtype)
            # (+ 8 u (|logdet| + n): the n rounded logs of the pivots themselves)
            tol_ld = 8 * n * kappa * U + 8 * U * (abs(want_ld[i]) + n) + out_rounding * abs(want_ld[i])
            assert abs(got_ld[i] - want_ld[i]) <= tol_ld, (transposed, i, got_ld[i], want_ld[i], kappa)
            assert abs(got_ld2[i] - want_ld[i]) <= tol_ld, (transposed, i, got_ld2[i], want_ld[i], kappa)
            scale = np.abs(want_inv[i]).max()
            err = np.abs(got_inv[i] - want_inv[i]).max()
            assert err <= (8 * n * kappa * U + out_rounding) * scale, (transposed, i, err, scale, kappa)


def test_inverse_spd_symmetrises_and_non_spd_gives_nan(ctx):
    rs = np.random.RandomState(3)
    n = 33
    A = _spd(rs, n, 100.0)
    K = rs.standard_normal((n, n))
    skew = 1e-7 * (K - K.T)                                # the two triangles differ by rounding-sized amounts
    Ad = ctx.to_device(np.stack([A + skew, A]))
    inv = ctx.zeros((2, n, n), torch.float64)
    ld = ctx.zeros(2, torch.float64)
    ctx.call("bsc_inverse_spd", 1, 2, n, Ad, n * n, n, 1, inv, ld)
    ctx.sync()
    got = inv.cpu().numpy()
    want = np.linalg.inv(A)                                # the mean of the two triangles of A + skew is A
    kappa = np.linalg.cond(A)
    assert np.abs(got[0] - want).max() <= 8 * n * kappa * U * np.abs(want).max()
    assert np.abs(got[0] - got[1]).max() <= 8 * n * kappa * U * np.abs(want).max()
    # not positive definite: one negative eigenvalue
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    lam = np.linspace(1.0, 2.0, n)
    lam[n // 2] = -0.5
    B = (Q * lam) @ Q.T
    B = 0.5 * (B + B.T)
    Bd = ctx.to_device(B[None])
    out = ctx.zeros(1, torch.float64)
    ctx.call("bsc_logdet_spd", 1, 1, n, Bd, n * n, n, 1, out)
    ctx.call("bsc_inverse_spd", 1, 1, n, Bd, n * n, n, 1, inv, ld)
    ctx.sync()
    assert np.isnan(out.item()) and np.isnan(ld[0].item())
    assert np.isnan(inv[0].cpu().numpy()).all()


def _elemwise(ctx, op, arrays, shape, out_view=None):
    """bsc_elemwise over `shape`: arrays are device tensors (views: strided / broadcast by stride 0 on extent 1)."""
    outbuf = torch.full([2 * s for s in shape], float("nan"), dtype=torch.float64, device=ctx.device)
    out = outbuf[tuple(slice(None, None, 2) for _ in shape)]           # every other element: strided
    strides = []
    for t in arrays:
        strides += [0 if t.shape[a] == 1 and shape[a] != 1 else t.stride(a) for a in range(len(shape))]
    ptrs = (ctypes.c_void_p * len(arrays))(*[t.data_ptr() for t in arrays])
    ctx.call("bsc_elemwise", OPS[op], 1, len(shape), _i64(shape), out, _i64(out.stride()), len(arrays), ptrs,
             _i64(strides))
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_in", range(1, 9))
def test_elemwise_float64_every_op_broadcast_and_strided(ctx, n_in):
    rs = np.random.RandomState(n_in)
    shape = [37, 5, 9]
    hosts, devs = [], []
    for i in range(n_in):
        if i % 3 == 1:                                     # broadcast over the middle axis
            h = rs.uniform(0.5, 2.0, (37, 1, 9))
            d = ctx.to_device(h)
        elif i % 3 == 2:                                   # a transposed view
            h = rs.uniform(0.5, 2.0, (9, 5, 37))
            d = ctx.to_device(h).permute(2, 1, 0)
            h = h.transpose(2, 1, 0)
        else:                                              # a strided slice
            h = rs.uniform(0.5, 2.0, (37, 10, 9))
            d = ctx.to_device(h)[:, ::2, :]
            h = h[:, ::2, :]
        hosts.append(h)
        devs.append(d)
    full = [np.broadcast_to(h, shape) for h in hosts]
    for op in ("add", "mul"):
        got = _elemwise(ctx, op, devs, shape)
        want = full[0].copy()
        for h in full[1:]:
            want = want + h if op == "add" else want * h
        assert np.abs(got - want).max() <= 4 * n_in * U * np.abs(want).max(), op
    unary = {"log": np.log, "exp": np.exp, "abs_": np.abs, "copy": lambda v: v}
    for op, f in unary.items():
        got = _elemwise(ctx, op, devs[:1], shape)
        want = f(full[0])
        assert np.all(np.abs(got - want) <= 4 * U * np.abs(want) + U), op       # (+ U: log next to 1)
    if n_in >= 2:
        got = _elemwise(ctx, "pow", devs[:2], shape)
        want = np.power(full[0], full[1])
        assert np.all(np.abs(got - want) <= 8 * U * np.abs(want))
    neg = ctx.to_device(-np.ascontiguousarray(hosts[0]))
    np.testing.assert_array_equal(_elemwise(ctx, "abs_", [neg], list(neg.shape)), np.abs(neg.cpu().numpy()))


def test_convert_round_trips_bit_exactly_through_permuted_and_strided_layouts(ctx):
    rs = np.random.RandomState(11)
    x = rs.standard_normal((6, 7, 129)).astype(np.float32) * np.float32(1e3)
    x.reshape(-1)[:4] = [np.float32(1e-45), np.float32(-3.4e38), np.float32(0.0), np.float32(-0.0)]
    src = ctx.to_device(x).permute(2, 0, 1)                # [129, 6, 7], permuted
    shape = list(src.shape)
    mid = torch.full((129, 12, 7), float("nan"), dtype=torch.float64, device=ctx.device)[:, ::2, :]   # strided
    ctx.call("bsc_convert", 0, 1, 3, _i64(shape), src, _i64(src.stride()), mid, _i64(mid.stride()))
    back_buf = torch.full((7, 6, 129 * 2), float("nan"), dtype=torch.float32, device=ctx.device)
    back = back_buf[:, :, ::2].permute(2, 1, 0)            # [129, 6, 7]: another permutation, strided
    ctx.call("bsc_convert", 1, 0, 3, _i64(shape), mid, _i64(mid.stride()), back, _i64(back.stride()))
    ctx.sync()
    want = x.transpose(2, 0, 1)
    np.testing.assert_array_equal(mid.cpu().numpy(), want.astype(np.float64))          # f32 -> f64 is exact
    np.testing.assert_array_equal(back.cpu().numpy().view(np.uint32), want.view(np.uint32))   # ... and back, bits
    # f64 -> f32 rounds to nearest even, as numpy does
    y = rs.standard_normal((33, 65)) * 10.0 ** rs.uniform(-40, 38, (33, 65))
    yd = ctx.to_device(y).t()
    out = torch.empty((65, 33), dtype=torch.float32, device=ctx.device)
    ctx.call("bsc_convert", 1, 0, 2, _i64(yd.shape), yd, _i64(yd.stride()), out, _i64(out.stride()))
    ctx.sync()
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), y.T.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("batch,M,N,K,ta,tb", [(3, 17, 33, 65, False, False), (2, 64, 1, 257, True, False),
                                               (5, 1, 129, 5, False, True), (1, 63, 65, 1, True, True),
                                               (4, 9, 7, 0, False, False), (70000, 2, 3, 4, False, True)])
def test_float64_gemm_strided_batched(ctx, batch, M, N, K, ta, tb):
    rs = np.random.RandomState(M * N + K)
    Ah = rs.standard_normal((batch, K, M) if ta else (batch, M, K))
    Bh = rs.standard_normal((batch, N, K) if tb else (batch, K, N))
    A, B = ctx.to_device(Ah), ctx.to_device(Bh)
    Av = A.transpose(1, 2) if ta else A
    Bv = B.transpose(1, 2) if tb else B
    Cbuf = torch.full((batch, M, N + 2), float("nan"), dtype=torch.float64, device=ctx.device)
    C = Cbuf[:, :, 1:N + 1]                                # row stride N + 2, offset one element
    ctx.call("bsc_gemm_strided_batched", 1, batch, M, N, K, Av, Av.stride(0), Av.stride(1), Av.stride(2),
             Bv, Bv.stride(0), Bv.stride(1), Bv.stride(2), C, C.stride(0), C.stride(1), C.stride(2))
    ctx.sync()
    a = np.swapaxes(Ah, 1, 2) if ta else Ah
    b = np.swapaxes(Bh, 1, 2) if tb else Bh
    want = np.einsum("bmk,bkn->bmn", a, b)
    bound = 2 * builtins.max(K, 1) * U * np.einsum("bmk,bkn->bmn", np.abs(a), np.abs(b))
    got = Cbuf.cpu().numpy()
    assert np.all(np.abs(got[:, :, 1:N + 1] - want) <= bound)
    assert np.isnan(got[:, :, 0]).all() and np.isnan(got[:, :, N + 1]).all()        # nothing outside C


# ---- special functions on the device: positive finite arguments only ---------------------------------------

def _map_unary(ctx, op, x):
    xd = ctx.to_device(x)
    out = torch.empty_like(xd)
    ptrs = (ctypes.c_void_p * 1)(xd.data_ptr())
    ctx.call("bsc_map_reduce", 1, OPS["add"], 1, _i64([x.size]), 0, _i64([]), 1, ptrs, _i64([1]), _i64([]),
             (ctypes.c_int32 * 1)(OPS[op]), (ctypes.c_double * 1)(0.0), 1.0, 0.0, OPS["copy"], 0.0, out, _i64([1]))
    ctx.sync()
    return out.cpu().numpy()


def test_digamma_and_gammaln_ops_in_float64_match_scipy(ctx):
    rs = np.random.RandomState(5)
    x = np.concatenate([np.logspace(-300, 300, 2001), np.linspace(1e-3, 20.0, 3001), rs.uniform(1.3, 1.6, 500),
                        [1.4616321449683623, 1.0, 2.0, 8.0, 7.999999999999999]])
    assert np.all(np.isfinite(x) & (x > 0))
    psi = _map_unary(ctx, "digamma", x)
    want = special.digamma(x)
    bad = ~(np.abs(psi - want) <= 1e-13 * np.abs(want) + 2e-15)
    assert not bad.any(), list(zip(x[bad][:5], psi[bad][:5], want[bad][:5]))
    lg = _map_unary(ctx, "gammaln", x)
    want = special.gammaln(x)
    bad = ~(np.abs(lg - want) <= 1e-13 * np.abs(want) + 2e-14)
    assert not bad.any(), list(zip(x[bad][:5], lg[bad][:5], want[bad][:5]))


def _dirichlet_ref(lam):
    lam64 = lam.astype(np.float64)
    return np.exp(special.digamma(lam64) - special.digamma(lam64.sum(1, keepdims=True)))


def _neg_kl(lam, prior):
    lam64 = lam.astype(np.float64)
    rows, cols = lam64.shape
    elog = special.digamma(lam64) - special.digamma(lam64.sum(1, keepdims=True))
    parts = [(prior - lam64) * elog, special.gammaln(lam64), -special.gammaln(lam64.sum(1)),
             np.full(rows, special.gammaln(cols * prior) - cols * special.gammaln(prior))]
    return builtins.sum(p.sum() for p in parts), builtins.sum(np.abs(p).sum() for p in parts)


@pytest.mark.parametrize("rows,cols,lo,hi", [(7, 333, -6, 6), (64, 1000, -30, 30), (3, 5, -3, 3), (300, 17, 0, 8)])
def test_dirichlet_expectation_and_bound_against_float64_scipy(ctx, rows, cols, lo, hi):
    rs = np.random.RandomState(rows + cols)
    lam = (10.0 ** rs.uniform(lo, hi, (rows, cols))).astype(np.float32)
    assert np.all(np.isfinite(lam) & (lam > 0))
    want = _dirichlet_ref(lam)
    d = ctx.to_device(lam)
    out = ctx.zeros((rows, cols))
    ctx.call("bsc_dirichlet_expectation", d, rows, cols, cols, out)
    out2 = ctx.zeros((rows, cols))
    bound = ctx.zeros(1, torch.float64)
    prior = 0.37
    ctx.call("bsc_dirichlet_expectation_bound", d, rows, cols, cols, prior, out2, bound)
    ctx.sync()
    tol = 2 * F32_ULP * want + 1e-45                        # the reference's float32 rounding and the kernel's
    for got in (out.cpu().numpy(), out2.cpu().numpy()):
        bad = ~(np.abs(got - want) <= tol)
        assert not bad.any(), list(zip(lam[bad][:5], got[bad][:5], want[bad][:5]))
    if hi <= 8:                                            # (the bound of a wide spread is dominated by one lnGamma)
        want_b, scale = _neg_kl(lam, prior)
        assert abs(bound.item() - want_b) <= 1e-13 * scale + 1e-12, (bound.item(), want_b, scale)
