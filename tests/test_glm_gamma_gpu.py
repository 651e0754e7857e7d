"""GPU parity of the Gamma route (csrc/bsc_glm_gamma.hip through the C ABI, svi/glm_gamma.py, svi/predict.py) against the
float64 restatement in tests/_glm_gamma_ref.py.

Tolerances are tests/test_glm_nb_gpu.py's with this likelihood's bound quantities:
 * ell: |dev - ref| <= 2e-5 * b_ell,  b_ell = sum_n v_n (|c_a| + alpha (|ly - l| + y e^{-l}) + |ly| + 1);
 * T:   |dev - ref| <= 2e-5 * b_T,    b_T   = sum_n v_n (alpha (|c_1| + |ly - l| + y e^{-l}) + 1);
 * G: rtol 1e-4, atol 1e-4 * max|G|; rows of weight 0 are left out of both sums;
 * extreme logits rtol 1e-6; exact power-of-two layouts and the zero-weight rows bit for bit;
 * the finish on supplied statistics rtol 1e-9, and the bits of bsc_glm_nb_update on the same arguments;
 * several updates against the reference: gradient 1e-4 * max|grad|, lam atol 2e-4, and the ELBO within 1e-6 of the
   sum of the absolute values of its terms (tests/_glm_gamma_ref.elbo_terms_size): the full density is in ell here,
   -log y included, and the ELBO can sit near zero, so -- by the cancellation tests/test_glm_nb_gpu.py describes -- a
   relative tolerance on the ELBO itself would ask the float32 pass for an arbitrary multiple of its accuracy;
 * the predictive: tests/_glm_gamma_ref.predict_bounds.
tau stays inside the accuracy envelope [-2.5, 5] (include/bayesic_hip.h).  A plain float32 evaluation of the same
formulas stays below 1e-6 of the bound quantities on these inputs (tests/test_glm_gamma_cpu.py), which leaves a factor
20 for the device's reduction order; the measured ratios are printed.

Shapes are the smallest that reach each path: B in {1, 7, 37, 16 k + 5}, D in {8, 64, 252, 256}, S in {1, 8, 11}
(11 = two launches, each with its own chunk of tau), ldx > D; at D = 256 the 16-row MFMA kernel with every vector
16-byte aligned and the 8-row kernel with each of y, o, v four bytes into its buffer; batches sized from the device's
CU count for 2 and 3 tiles per wave; sentinels of 1e30 behind y, o, v and logshape."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_gamma_ref as ref
import _glm_obs_ref as obs

pytestmark = pytest.mark.gpu

MODES = ("none", "offset", "weights", "both")
SENTINEL = 1.0e30      # behind the end of y / o / v / logshape: a read past the end would wreck the sums


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, W, logshape, o=None, v=None, ld=None, shift=()):
    B, D = X.shape
    S = W.shape[0]
    if ld is not None:
        buf = np.full((B, ld), 7.0, np.float32)         # the padding must never be read as data
        buf[:, :D] = X
        Xd = ctx.to_device(buf)
    else:
        Xd = ctx.to_device(X)
    Wd = ctx.to_device(W)
    yd, od, vd = (_dev_vec(ctx, a, k in shift) for k, a in (("y", y), ("o", o), ("v", v)))
    pd = _dev_vec(ctx, logshape, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    ctx.call("bsc_glm_gamma_data_pass", Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _assert_close(got, X, y, W, logshape, o, v, what=""):
    ell, G, T = got
    ell_r, G_r, T_r = ref.data_pass(X, y, W, logshape, o, v)
    b_ell, b_T = ref.bounds(X, y, W, logshape, o, v)
    e_ell, e_T = np.abs(ell - ell_r), np.abs(T - T_r)
    print("%s B=%d D=%d S=%d: ell err/bound %.3g, T err/bound %.3g, G err/max %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], (e_ell / (2e-5 * b_ell + 1e-300)).max(),
        (e_T / (2e-5 * b_T + 1e-300)).max(), np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300)))
    assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(T).all()
    assert (e_ell <= 2e-5 * b_ell + 1e-12).all(), (e_ell / (b_ell + 1e-300)).max()
    assert (e_T <= 2e-5 * b_T + 1e-12).all(), (e_T / (b_T + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())


def _check(ctx, X, y, W, logshape, o, v, **kw):
    assert -2.5 <= logshape.min() and logshape.max() <= 5.0
    got = _pass(ctx, X, y, W, logshape, o, v, **kw)
    _assert_close(got, X, y, W, logshape, o, v)
    return got


# ---- 1. parity over the envelope ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,ld", [(1, 8, 1, None), (7, 8, 8, 12), (37, 64, 11, None), (53, 64, 8, 96),
                                      (7, 252, 8, None), (165, 252, 11, 256), (1, 256, 8, None), (7, 256, 1, None),
                                      (37, 256, 8, 260), (325, 256, 11, None), (1029, 256, 8, 512)])
@pytest.mark.parametrize("mode", MODES)
def test_pass_matches_the_reference(ctx, mode, B, D, S, ld):
    X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode)
    _check(ctx, X, y, W, logshape, o, v, ld=ld)


@pytest.mark.parametrize("shift", [(), ("y",), ("o",), ("v",), ("p",), ("y", "o", "v", "p")])
def test_full_width_with_aligned_and_misaligned_vectors(ctx, shift):
    """D = 256: every vector 16-byte aligned takes the 16-row MFMA kernel, any one of y, o, v four bytes in the 8-row
    kernel; logshape is read four bytes at a time by both and may sit anywhere."""
    X, y, W, logshape, o, v = ref.make_inputs(1003, 256, 8, seed=3)
    _check(ctx, X, y, W, logshape, o, v, shift=shift)


# ---- 2. several tiles per wave ------------------------------------------------------------------------------------------

def _grid(B, rows, cu):
    n_tiles = (B + rows - 1) // rows
    max_waves = 8 * cu
    return (n_tiles + max_waves - 1) // max_waves


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("kernel,D,n_iter", [("mfma", 256, 2), ("mfma", 256, 3), ("valu", 256, 2), ("valu", 64, 3),
                                             ("valu", 252, 2)])
def test_several_tiles_per_wave_keep_T_and_the_per_draw_scalars(ctx, cu, kernel, D, n_iter):
    """B = (n_iter - 1) sweeps of the resident waves + one tile + 5 rows (tests/test_glm_nb_gpu.py's form): T and the
    draw's tau, alpha, c_a, c_1 have to survive the hand-over from one tile to the next.  Every draw has its own tau,
    every row its own offset and weight."""
    rows = 16 if kernel == "mfma" else 8
    B = (n_iter - 1) * 8 * cu * rows + rows + 5
    assert _grid(B, rows, cu) == n_iter
    rs = np.random.RandomState(n_iter + D)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, D))).astype(np.float32)
    logshape = np.linspace(-2.5, 5.0, 8).astype(np.float32)[rs.permutation(8)]
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)          # distinct within any two tiles of a wave
    v = (0.25 + (np.arange(B) % 1013) / 500.0).astype(np.float32)
    v[::7] = 0.0
    y = (0.125 + 0.5 * (np.arange(B) % 5) + 0.01 * (np.arange(B) % 3)).astype(np.float32)
    y[::101] = 750.0
    y[50::103] = 1.0e-3
    shift = ("y",) if (kernel == "valu" and D == 256) else ()
    _check(ctx, X, y, W, logshape, o, v, shift=shift)


# ---- 3. exact layout ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,B,shift,weights", [(256, 600, (), False), (256, 600, ("y",), True), (64, 200, (), True)])
def test_exact_row_accounting(ctx, D, B, shift, weights):
    """W = 0, o = 0, tau = 0 and one-hot X (row n has its 1 in column n mod D): l = 0, e^{-l} = 1 and alpha = 1 exactly, so
    r = v (y - 1) and column d of G is the sum of it over the rows of column d, for every draw.  y and v are powers of
    two (y from 1/16 to 64, v from 1/4 to 1): multiples of 1/64 below 2^9, exact in float32 in any order and checked bit
    for bit -- any row / draw / column mix-up shows."""
    S = 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    W = np.zeros((S, D), np.float32)
    logshape = np.zeros(S, np.float32)
    y = (2.0 ** (((np.arange(B) * 7) % 11) - 4)).astype(np.float32)
    v = (2.0 ** -((np.arange(B) * 2) % 3)).astype(np.float32) if weights else None
    if weights:
        v[::13] = 0.0
    _, G, _ = _pass(ctx, X, y, W, logshape, None, v, shift=shift)
    term = (1.0 if v is None else v.astype(np.float64)) * (y.astype(np.float64) - 1.0)
    want = np.zeros(D)
    np.add.at(want, np.arange(B) % D, term)
    npt.assert_array_equal(G, np.broadcast_to(want, (S, D)))
    assert len(set(want)) > 12


# ---- 4. extremes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
def test_extreme_logits_through_the_offset_are_finite(ctx, D, B):
    """Integer logits +-80 of which +-75 come from the offset (and +-70 with the offset flipped): y e^{-l} up to 8 e^80
    = 4e35, finite in float32, and everything at rtol 1e-6 -- the exponential is the product y e^{-l}, not
    e^{log y - l}, whose rounded argument would cost 4e-6 there.  tau = 0, so alpha = 1, c_a = 0 and c_1 = 1 + gamma are
    exact or one rounding; y is a power of two."""
    S = 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(D)[None, :])
    W = (5.0 * sign).astype(np.float32)
    logshape = np.zeros(S, np.float32)
    y = np.array([0.25, 1.0, 2.0, 8.0], np.float32)[(np.arange(B) // 2) % 4]
    v = (1.0 + (np.arange(B) % 3)).astype(np.float32)
    for flip in (1.0, -1.0):
        o = (flip * 75.0 * sign[0, np.arange(B) % D]).astype(np.float32)
        L = obs.logits(X, W, o)
        assert set(np.unique(np.abs(L[:, 0]))) == ({80.0} if flip > 0 else {70.0})
        assert (L[:, 0] > 0).any() and (L[:, 0] < 0).any()
        ell, G, T = _pass(ctx, X, y, W, logshape, o, v)
        assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(T).all()
        ell_r, G_r, T_r = ref.data_pass(X, y, W, logshape, o, v)
        npt.assert_allclose(ell, ell_r, rtol=1e-6)
        npt.assert_allclose(G, G_r, rtol=1e-6)
        npt.assert_allclose(T, T_r, rtol=1e-6)


# ---- 5. zero-weight rows and the tail tile ----------------------------------------------------------------------------------

@pytest.mark.parametrize("D,shift", [(256, ()), (256, ("o",)), (64, ())])
def test_zero_weight_rows_with_wild_terms_add_exactly_nothing(ctx, D, shift):
    """37 rows, then three more of weight 0 whose y and offset are wild (1e30, 1e-30, 3e38; a logit of 200, -1e30, 1e30).
    37 and 40 rows make the same tiles and the same grid in both kernels, so the pass over 40 rows must return the bits
    of the pass over 37: the wild rows are dropped by a select, not multiplied away."""
    X, y, W, logshape, o, v = ref.make_inputs(40, D, 8, seed=D + 1)
    v[37:] = 0.0
    v[36] = 1.5
    y[37:] = [1.0e30, 1.0e-30, 3.0e38]
    o[37:] = [200.0, -1.0e30, 1.0e30]
    a = _pass(ctx, X, y, W, logshape, o, v, shift=shift)
    b = _pass(ctx, X[:37], y[:37], W, logshape, o[:37], v[:37], shift=shift)
    for got, want, name in zip(a, b, ("ell", "G", "T")):
        assert np.isfinite(got).all(), name
        npt.assert_array_equal(got, want, err_msg=name)
    _assert_close(a, X[:37], y[:37], W, logshape, o[:37], v[:37], what="rows removed")


@pytest.mark.parametrize("D,B,shift", [(256, 13, ()), (256, 21, ()), (256, 13, ("y",)), (64, 3, ()), (8, 9, ())])
@pytest.mark.parametrize("mode", ["none", "both"])
def test_a_tail_tile_past_the_batch_forms_no_log_of_zero(ctx, mode, D, B, shift):
    """The last tile reads y = 0 past B through its descriptor (without weights nothing but the row count masks it):
    every sum is finite and the reference's."""
    X, y, W, logshape, o, v = ref.make_inputs(B, D, 8, seed=B + D, mode=mode)
    _check(ctx, X, y, W, logshape, o, v, shift=shift)


def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (165, 64, 8, 6)):
        X, y, W, logshape, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, logshape, o, v)
        b = _pass(ctx, X, y, W, logshape, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


def test_an_empty_batch_gives_zeros(ctx):
    S, D = 11, 64
    W, logshape = ctx.zeros((S, D)), ctx.zeros(S)
    ell, G, T = (torch.full(s, 7.0, dtype=torch.float64, device=ctx.device) for s in ((S,), (S, D), (S,)))
    ctx.call("bsc_glm_gamma_data_pass", None, D, None, None, None, 0, D, W, logshape, S, ell, G, T)
    ctx.sync()
    assert not ell.any() and not G.any() and not T.any()


# ---- 6. the finish ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S", [(256, 8), (64, 11), (8, 1)])
def test_finish_on_supplied_statistics(ctx, D, S):
    """bsc_glm_gamma_update against tests/_glm_gamma_ref.update on the same float64 statistics: everything is float64 on
    both sides, rtol 1e-9; the next draws are those float64 values rounded to float32.  bsc_glm_nb_update on the same
    arguments returns the same bits: the two entry points run one body."""
    f64 = torch.float64
    P = D + 1
    rs = np.random.RandomState(D + S)
    seed, t = 77, 4
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, logshape = ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(2 * P), 0.01 * rs.uniform(size=2 * P)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, m1_r, m2_r, elbo_r, grad_r = ref.update(lam, m1.copy(), m2.copy(), t, eps, W, logshape, ell, G, T, scale, prec,
                                                   a0, b0, lr)

    def run(name):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W=ctx.to_device(W.ravel()), lp=_dev_vec(ctx, logshape),
                 W_n=ctx.zeros(S * D), lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64),
                 stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
        ctx.call(name, d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["lp"], D, S, scale, prec,
                 a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"], d["elbo"], d["grad"])
        ctx.sync()
        return {k: a.cpu().numpy() for k, a in d.items()}

    h = run("bsc_glm_gamma_update")
    npt.assert_allclose(h["elbo"][0], elbo_r, rtol=1e-9)
    npt.assert_allclose(h["grad"], grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
    npt.assert_allclose(h["out"], lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(h["m1"], m1_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(h["m2"], m2_r, rtol=1e-9, atol=1e-15)
    npt.assert_array_equal(h["lam"], lam)                      # lam_in is not modified
    W_n, lp_n = ref.draw(lam_r, eps_n)
    npt.assert_allclose(h["W_n"].reshape(S, D), W_n, rtol=2e-7, atol=1e-9)
    npt.assert_allclose(h["lp_n"], lp_n, rtol=2e-7, atol=1e-9)
    twin = run("bsc_glm_nb_update")
    for k in ("elbo", "grad", "out", "m1", "m2", "W_n", "lp_n"):
        npt.assert_array_equal(h[k], twin[k], err_msg=k)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------------

def _regression_data(B, D, seed, alpha=3.0, shift=0.5):
    """tests/test_glm_obs_gpu.py's regression data with a Gamma response of shape ``alpha``."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.5 * rs.standard_normal(B) + shift).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    mu = np.exp(X.astype(np.float64) @ rs.standard_normal(D) + o)
    y = np.maximum(rs.gamma(alpha, mu / alpha), 1.0e-30).astype(np.float32)
    return X, y, o, v


def _run_twenty(ctx, S, check):
    from bayesic_amd.svi import GammaReparamSVI
    B, D, seed, lr, prec, a0, b0 = 1029, 256, 1234, 0.01, 2.0, 1.5, 0.5
    batches = [_regression_data(B, D, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, y0, o0, v0 = dev[0]
    model = GammaReparamSVI(X0, y0, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0, b0=b0,
                            ctx=ctx, offset=o0, weights=v0)
    lam = ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 21):
            k = (t - 1) % 2
            Xk, yk, ok, vk = dev[k]
            model.set_batch(Xk, yk, offset=ok, weights=vk)
            assert model.step() is None
            if not check:
                continue
            Xh, yh, oh, vh = batches[k]
            W_r, lp_r = ref.draw(lam, ref.noise(D, S, seed, t - 1))
            rho = lam[D + 1:].copy()
            lam, m1, m2, elbo, grad = ref.step(lam, m1, m2, t, Xh, yh, S, seed, 10.0 * B, lr, prec, a0, b0, offset=oh,
                                               weights=vh)
            if t in (1, 2, 3, 10, 20):
                size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(Xh, yh, W_r, lp_r, oh, vh)[0], 10.0, prec, a0, b0, rho)
                ctx.sync()
                g = model.grad.cpu().numpy()
                e = abs(model.elbo.item() - elbo)
                print("t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g" % (
                    t, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max()))
                assert e <= 1e-6 * size, (e, size)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    ctx.sync()
    return model, lam, calls


@pytest.mark.parametrize("S", [8, 11])
def test_twenty_updates_track_the_reference_over_two_batches(ctx, S):
    model, lam, calls = _run_twenty(ctx, S, check=True)
    D = model.D
    assert "bsc_glm_gamma_data_pass" in calls and "bsc_glm_gamma_update" in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_gamma_" not in c]
    p = model.params()
    npt.assert_allclose(p["shape_mean"], math.exp(lam[D] + 0.5 * math.exp(2.0 * lam[2 * D + 1])), rtol=1e-3)


def test_two_driver_runs_from_one_seed_give_the_same_bits(ctx):
    a, _, _ = _run_twenty(ctx, 8, check=False)
    b, _, _ = _run_twenty(ctx, 8, check=False)
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    npt.assert_array_equal(a.elbo.cpu().numpy(), b.elbo.cpu().numpy())
    npt.assert_array_equal(a.grad.cpu().numpy(), b.grad.cpu().numpy())


def test_driver_checks_the_batch_outside_step(ctx):
    from bayesic_amd.svi import GammaReparamSVI
    B, D = 325, 64
    X, y, o, v = _regression_data(B, D, 7)
    Xd, yd, od, vd = (ctx.to_device(a) for a in (X, y, o, v))
    with pytest.raises(ValueError, match="y must be finite and > 0"):
        GammaReparamSVI(Xd, yd - yd[0], ctx=ctx)                      # one exact zero
    m = GammaReparamSVI(Xd, yd, ctx=ctx, exposure=np.exp(o))
    npt.assert_allclose(m.offset.cpu().numpy(), o, rtol=1e-5, atol=1e-6)           # kept as log(exposure)
    assert m.has_offset
    bad = yd.clone()
    bad[5] = float("nan")
    with pytest.raises(ValueError, match="y must be finite and > 0"):
        m.set_batch(Xd, bad)
    bad[5] = 0.0
    with pytest.raises(ValueError, match="y must be finite and > 0"):
        m.set_batch(Xd, bad)
    with pytest.raises(ValueError, match="finite and >= 0"):
        m.set_batch(Xd, yd, weights=-vd - 1.0)
    m.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())   # taken as they are
    m.step()
    m2 = GammaReparamSVI(Xd, yd, ctx=ctx, offset=od, weights=vd)
    m2.step()
    ctx.sync()
    npt.assert_array_equal(m.lam.cpu().numpy(), m2.lam.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        m2.predict(Xd, yd)


# ---- 8. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, logshape, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, logshape, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call("bsc_gamma_predict_pass", Xd, D, yd, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, logshape, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, logshape, y, o, v)
    bnd = ref.predict_bounds(X, W, logshape, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        print("gamma %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    """make_inputs with the logits kept at |l| <= 3.5 (the predictive mean is exp(l), as for the Poisson family)."""
    X, y, W, logshape, o, _ = ref.make_inputs(B, D, S, seed, mode="offset")
    peak = np.abs(obs.logits(X, W, o)).max()
    if peak > 3.5:
        W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    return X, y, W, logshape, (o if offset else None)


@pytest.mark.parametrize("B,D,S,shift,offset", [(1, 64, 1, False, True), (37, 64, 16, False, False),
                                                (53, 64, 33, True, True), (165, 64, 64, False, True),
                                                (37, 256, 1, True, True), (1003, 256, 16, False, False),
                                                (325, 256, 33, False, True), (1003, 256, 64, True, True)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset):
    X, y, W, logshape, o = _predict_inputs(B, D, S, B + D + S, offset)
    got = _predict(ctx, X, y, W, logshape, o, shift=shift)
    _assert_predict(got, X, y, W, logshape, o)


def test_predict_optional_outputs(ctx):
    X, y, W, logshape, o = _predict_inputs(165, 64, 16, 9)
    full = _predict(ctx, X, y, W, logshape, o)
    for want in (("mean",), ("var",), ("lpd",), ("lpd_sum",), ("mean", "lpd_sum")):
        got = _predict(ctx, X, y, W, logshape, o, want=want)
        for k in ("mean", "var", "lpd", "lpd_sum"):
            if k in want:
                npt.assert_array_equal(got[k], full[k], err_msg=k)
            else:
                assert (got[k] == -777.0).all(), k
    # without y: the moments alone
    B, D = X.shape
    mean = torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device)
    ctx.call("bsc_gamma_predict_pass", ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W),
             _dev_vec(ctx, logshape), 16, mean, None, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])


def test_predict_several_tiles_per_wave_pairs_every_row_with_its_offset(ctx, cu):
    B = 8 * cu * 16 + 16 + 5
    rs = np.random.RandomState(2)
    X = (rs.standard_normal((B, 256)) / 16.0).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, 256))).astype(np.float32)
    logshape = np.linspace(-2.5, 5.0, 8).astype(np.float32)
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)
    y = (0.125 + 0.5 * (np.arange(B) % 7) + 0.25 * (np.arange(B) % 2)).astype(np.float32)
    got = _predict(ctx, X, y, W, logshape, o)
    _assert_predict(got, X, y, W, logshape, o)


def test_driver_predict_with_exposure_and_weights(ctx):
    from bayesic_amd.svi import GammaReparamSVI
    from bayesic_amd.svi import predict as mod
    rs = np.random.RandomState(12)
    B, D = 600, 8
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    expo = np.exp(rs.uniform(math.log(0.1), math.log(10.0), B)).astype(np.float32)
    mu = expo * np.exp(X.astype(np.float64) @ (0.5 * rs.standard_normal(D)))
    y = np.maximum(rs.gamma(2.0, mu / 2.0), 1.0e-30).astype(np.float32)
    m = GammaReparamSVI(X, y, exposure=expo, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "gamma"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    draws = mod.posterior_draws(m, 16)
    W, logshape = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(logshape, lp_r)
    o = m.offset.cpu().numpy()
    out = m.predict(X, y, exposure=expo, draws=draws)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _assert_predict(got, X, y, W, logshape, o)
    assert m.heldout_lpd(X, y, exposure=expo, draws=draws) == float(out["lpd_sum"].item()) / B
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, logshape, o, v)
    score = m.heldout_lpd(X, y, exposure=expo, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    assert float(wout["weight_sum"].item()) == float(v.astype(np.float64).sum())
    # a model fitted without an offset predicts without one
    m0 = GammaReparamSVI(X, y, n_samples=8, seed=9, ctx=ctx)
    m0.step()
    d0 = mod.posterior_draws(m0, 33)
    g0 = {k: t.cpu().numpy() for k, t in m0.predict(X, y, draws=d0).items()}
    _assert_predict(g0, X, y, d0[0].cpu().numpy(), d0[1].cpu().numpy(), None)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9) + 1.0, ctx.zeros((65, 260))
    o, v, lp = ctx.zeros(12), ctx.zeros(12), ctx.zeros(68)
    ell, G, T = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros(65, f64)

    def call(Xa, ldx, D, S, Wa=W, pa=lp, ya=y, B=8, oa=o, va=v):
        ctx.call("bsc_glm_gamma_data_pass", Xa, ldx, ya, oa, va, B, D, Wa, pa, S, ell, G, T)

    # the training pass refuses with bsc_glm_nb_data_pass's checks, code and all
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: D=6 must be a multiple of 4"):
        call(X, 8, 6, 8)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: D=260 must be a multiple of 4 in"):
        call(X, 260, 260, 8)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: S=65"):
        call(X, 256, 256, 65)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: X and W must be 16-byte aligned"):
        call(X.view(-1)[1:], 256, 256, 8)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: X and W must be 16-byte aligned"):
        call(X, 256, 256, 8, Wa=W.view(-1)[1:])
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: ldx=6"):
        call(X, 6, 8, 8)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: logshape is null"):
        call(X, 256, 256, 8, pa=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: logshape must be 4-byte aligned"):
        call(X, 256, 256, 8, pa=lp.data_ptr() + 2)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: offset and weight must be 4-byte aligned"):
        call(X, 256, 256, 8, oa=o.data_ptr() + 2)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: y is null with B=8"):
        call(X, 256, 256, 8, ya=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_data_pass: null output"):
        ctx.call("bsc_glm_gamma_data_pass", X, 256, y, o, v, 8, 256, W, lp, 8, ell, G, None)

    lam, m = ctx.zeros((2, 18), f64), ctx.zeros((2, 18), f64)
    eps = ctx.zeros((2, 8 * 9), f64)
    stats = ctx.zeros(8 * 10, f64)
    Wn, pn = ctx.zeros(8 * 8), ctx.zeros(8)

    def update(st=stats, S=8, a0=1.0, b0=1.0, tau=1.0, scale=1.0, t=1, p_next=pn, p=lp):
        ctx.call("bsc_glm_gamma_update", st, lam[0], lam[1], m[0], m[1], eps[0], W, p, 8, S, scale, tau, a0, b0, t, 0.01,
                 0.9, 0.999, 1e-8, 1, 1, eps[1], 1, Wn, p_next, ell, G)

    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: stats is null"):
        update(st=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: null pointer"):
        update(p=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: a0=0 b0=1 must be positive"):
        update(a0=0.0)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: a0=1 b0=-2 must be positive"):
        update(b0=-2.0)
    with pytest.raises(BayesicHipError, match=r"bsc_glm_gamma_update: D=8 S=65 \(S<=64\)"):
        update(S=65)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: prior_precision=0 must be positive"):
        update(tau=0.0)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: scale=0 must be positive"):
        update(scale=0.0)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: the Adam step count starts at 1"):
        update(t=0)
    with pytest.raises(BayesicHipError, match="bsc_glm_gamma_update: next-draw buffers must be all set or all null"):
        update(p_next=None)

    out = ctx.zeros(9)

    def predict(D=8, S=8, Xa=X, ya=y, pa=lp, ldx=8, outs=(out, None, None, None)):
        ctx.call("bsc_gamma_predict_pass", Xa, ldx, ya, o, 8, D, W, pa, S, *outs)

    with pytest.raises(BayesicHipError, match="bsc_gamma_predict_pass: logshape is null"):
        predict(pa=None)
    with pytest.raises(BayesicHipError, match="bsc_gamma_predict_pass: offset and logshape must be 4-byte aligned"):
        predict(pa=lp.data_ptr() + 2)
    with pytest.raises(BayesicHipError, match="bsc_gamma_predict_pass: lpd and lpd_sum need y"):
        predict(ya=None, outs=(None, None, out, None))
    with pytest.raises(BayesicHipError, match="bsc_gamma_predict_pass: no output requested"):
        predict(outs=(None, None, None, None))
    for kw, match in ((dict(S=65), "bsc_gamma_predict_pass: S=65"),
                      (dict(D=6), "bsc_gamma_predict_pass: D=6 must be a multiple of 4"),
                      (dict(D=260, ldx=260), "bsc_gamma_predict_pass: D=260 must be a multiple of 4"),
                      (dict(Xa=X.view(-1)[1:]), "bsc_gamma_predict_pass: X and W must be 16-byte aligned")):
        with pytest.raises(BayesicHipError, match=match) as err:
            predict(**kw)
        assert "status -3:" in str(err.value), str(err.value)          # BSC_ERR_UNSUPPORTED
    ctx.sync()
