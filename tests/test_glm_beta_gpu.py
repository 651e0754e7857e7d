"""GPU parity of the Beta route (csrc/bsc_glm_beta.hip through the C ABI, svi/glm_beta.py, svi/predict.py) against the
float64 restatement in tests/_glm_beta_ref.py.

Tolerances are tests/test_glm_nb_gpu.py's with this likelihood's bound quantities (tests/_glm_beta_ref.py's docstring):
 * ell: |dev - ref| <= 2e-5 * b_ell,  b_ell = sum_n v (|lnGamma phi| + S(a) + S(b) + |log min(a, 1)| + |log min(b, 1)|
                                                     + (a + 1)|ly| + (b + 1)|l1y| + 1);
 * T:   |dev - ref| <= 2e-5 * b_T,    b_T   = sum_n v (phi (|psi phi| + m (|ly| + |psi a|) + (1 - m)(|l1y| + |psi b|)) + 1);
 * G: rtol 1e-4, atol 1e-4 * max|G|; rows of weight 0 are left out of both sums;
 * logits of +-80 and +-70: everything finite and inside the same bound-based tolerances (not rtol 1e-6: T at tau = 5
   cancels from 2e3 per row down to O(1));
 * y = 1/2, tau = log 2 on one-hot rows: G exactly 0; the zero-weight rows bit for bit;
 * the finish on supplied statistics rtol 1e-9, and the bits of bsc_glm_nb_update on the same arguments; the
   full-covariance finish on the driver's own statistics rtol 1e-9 against tests/_glm_scalar_full_ref.py;
 * several updates against the reference, both guides: gradient 1e-4 * max|grad|, lam atol 2e-4, and the ELBO within
   1e-6 of the sum of the absolute values of its terms (tests/_glm_beta_ref.elbo_terms_size);
 * recovery of a simulated precision of 20 within 15 % (the float64 reference alone lands at 19.89 on the same data and
   draws, tests/test_glm_beta_cpu.py; so does the device);
 * the predictive: tests/_glm_beta_ref.predict_bounds.
tau stays inside the accuracy envelope [-2, 5] (include/bayesic_hip.h).  A plain float32 evaluation of the kernel's
formulas stays below 1e-6 of the bound quantities on these inputs (tests/test_glm_beta_cpu.py), which leaves a factor 20
for the device's reduction order; the measured ratios are printed (on one MI355X: ell and T within 0.7 % of their
tolerances, G within 1.9e-6 of its maximum).

Shapes are the smallest that reach each path: B in {1, 7, 37, 16 k + 5}, D in {8, 64, 252, 256}, S in {1, 8, 11}
(11 = two launches, each with its own chunk of tau), ldx > D; at D = 256 the 16-row MFMA kernel with every vector
16-byte aligned and the 8-row kernel with each of y, o, v four bytes into its buffer; batches sized from the device's
CU count for 2 and 3 tiles per wave; sentinels of 1e30 behind y, o, v and logprec."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_beta_ref as ref
import _glm_obs_ref as obs
import _glm_scalar_full_ref as full_ref

pytestmark = pytest.mark.gpu

MODES = ("none", "offset", "weights", "both")
SENTINEL = 1.0e30      # behind the end of y / o / v / logprec: a read past the end would wreck the sums


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, X, y, W, logprec, o=None, v=None, ld=None, shift=()):
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
    pd = _dev_vec(ctx, logprec, "p" in shift)
    ell, G, T = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64), ctx.zeros(S, torch.float64)
    ctx.call("bsc_glm_beta_data_pass", Xd, (ld or D), yd, od, vd, B, D, Wd, pd, S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _assert_close(got, X, y, W, logprec, o, v, what=""):
    ell, G, T = got
    ell_r, G_r, T_r = ref.data_pass(X, y, W, logprec, o, v)
    b_ell, b_T = ref.bounds(X, y, W, logprec, o, v)
    e_ell, e_T = np.abs(ell - ell_r), np.abs(T - T_r)
    print("%s B=%d D=%d S=%d: ell err/bound %.3g, T err/bound %.3g, G err/max %.3g" % (
        what, X.shape[0], X.shape[1], W.shape[0], (e_ell / (2e-5 * b_ell + 1e-300)).max(),
        (e_T / (2e-5 * b_T + 1e-300)).max(), np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300)))
    assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(T).all()
    assert (e_ell <= 2e-5 * b_ell + 1e-12).all(), (e_ell / (b_ell + 1e-300)).max()
    assert (e_T <= 2e-5 * b_T + 1e-12).all(), (e_T / (b_T + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())


def _check(ctx, X, y, W, logprec, o, v, **kw):
    assert ref.TAU_LO <= logprec.min() and logprec.max() <= ref.TAU_HI
    got = _pass(ctx, X, y, W, logprec, o, v, **kw)
    _assert_close(got, X, y, W, logprec, o, v)
    return got


# ---- 1. parity over the envelope ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,ld", [(1, 8, 1, None), (7, 8, 8, 12), (37, 64, 11, None), (53, 64, 8, 96),
                                      (7, 252, 8, None), (165, 252, 11, 256), (1, 256, 8, None), (7, 256, 1, None),
                                      (37, 256, 8, 260), (325, 256, 11, None), (1029, 256, 8, 512)])
@pytest.mark.parametrize("mode", MODES)
def test_pass_matches_the_reference(ctx, mode, B, D, S, ld):
    X, y, W, logprec, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S, mode=mode)
    _check(ctx, X, y, W, logprec, o, v, ld=ld)


@pytest.mark.parametrize("shift", [(), ("y",), ("o",), ("v",), ("p",), ("y", "o", "v", "p")])
def test_full_width_with_aligned_and_misaligned_vectors(ctx, shift):
    """D = 256: every vector 16-byte aligned takes the 16-row MFMA kernel, any one of y, o, v four bytes in the 8-row
    kernel; logprec is read four bytes at a time by both and may sit anywhere."""
    X, y, W, logprec, o, v = ref.make_inputs(1003, 256, 8, seed=3)
    _check(ctx, X, y, W, logprec, o, v, shift=shift)


# ---- 2. several tiles per wave ------------------------------------------------------------------------------------------

def _grid(B, rows, cu):
    n_tiles = (B + rows - 1) // rows
    max_waves = 8 * cu
    return (n_tiles + max_waves - 1) // max_waves


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("kernel,D,n_iter", [("mfma", 256, 2), ("mfma", 256, 3), ("valu", 256, 2), ("valu", 256, 3),
                                             ("valu", 64, 3), ("valu", 252, 2)])
def test_several_tiles_per_wave_keep_T_and_the_per_draw_scalars(ctx, cu, kernel, D, n_iter):
    """B = (n_iter - 1) sweeps of the resident waves + one tile + 5 rows (tests/test_glm_nb_gpu.py's form): T and the
    draw's tau, phi, lnGamma(phi), psi(phi) have to survive the hand-over from one tile to the next.  Every draw has its
    own tau spread over [-2, 5], every row its own offset and weight; y cycles through seven values from 1e-6 to
    1 - 1e-6."""
    rows = 16 if kernel == "mfma" else 8
    B = (n_iter - 1) * 8 * cu * rows + rows + 5
    assert _grid(B, rows, cu) == n_iter
    rs = np.random.RandomState(n_iter + D)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, D))).astype(np.float32)
    logprec = np.linspace(ref.TAU_LO, ref.TAU_HI, 8).astype(np.float32)[rs.permutation(8)]
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)          # distinct within any two tiles of a wave
    v = (0.25 + (np.arange(B) % 1013) / 500.0).astype(np.float32)
    v[::7] = 0.0
    y = np.array([ref.Y_LO, 0.01, 0.2, 0.5, 0.7, 0.97, ref.Y_HI], np.float32)[np.arange(B) % 7]
    shift = ("y",) if (kernel == "valu" and D == 256) else ()
    _check(ctx, X, y, W, logprec, o, v, shift=shift)


# ---- 3. exact layout ------------------------------------------------------------------------------------------------------

def _one_hot(B, D):
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    return X


@pytest.mark.parametrize("D,B,shift,weights", [(256, 600, (), False), (256, 600, ("y",), True), (64, 200, (), True)])
def test_exact_row_accounting_at_the_uniform_density(ctx, D, B, shift, weights):
    """W = 0, o = 0, tau = log 2 and y = 1/2 on one-hot X: l = 0, e = 1, m = 1 - m = 1/2 and phi = 2 exactly (expf of the
    float32 log 2 rounds to 2), so a = b = 1 in every lane.  psi(a) and psi(b) are then the same bits, ly and l1y as well
    (log1p(-y) = log(w) * y / (1 - w) with w = 1/2: the quotient is exactly 1), and r = v phi / 4 ((ly - l1y) - psi(a) +
    psi(b)) is an exact 0: G == 0 bit for bit, for every draw, whatever the weights.
    ell: Beta(1, 1) is the uniform density and the reference's ell is zero (to the 2e-9 by which e^tau misses 2 in
    float64).  The device's lnGamma(1) is the float32 difference Stirling(8) - log 5040 of two values of size 8.5, zero to
    an ulp of those and not exactly: ell is held to 2e-5 b_ell like everywhere else, and to the same bits in every
    draw."""
    S = 8
    X = _one_hot(B, D)
    W = np.zeros((S, D), np.float32)
    logprec = np.full(S, math.log(2.0), np.float32)
    y = np.full(B, 0.5, np.float32)
    v = (2.0 ** -((np.arange(B) * 2) % 3)).astype(np.float32) if weights else None
    if weights:
        v[::13] = 0.0
    ell, G, T = _pass(ctx, X, y, W, logprec, None, v, shift=shift)
    npt.assert_array_equal(G, np.zeros((S, D)))
    b_ell, b_T = ref.bounds(X, y, W, logprec, None, v)
    ell_r, _, T_r = ref.data_pass(X, y, W, logprec, None, v)
    print("ell / bound quantity %.3g (reference %.3g)" % (np.abs(ell / b_ell).max(), np.abs(ell_r / b_ell).max()))
    assert np.abs(ell_r).max() <= 1e-9 * b_ell.max()
    assert (np.abs(ell - ell_r) <= 2e-5 * b_ell).all()
    assert (np.abs(T - T_r) <= 2e-5 * b_T).all()
    assert (ell == ell[0]).all() and (T == T[0]).all()


@pytest.mark.parametrize("D,B,shift", [(256, 600, ()), (256, 600, ("o",)), (64, 200, ())])
def test_columns_of_G_belong_to_their_rows_and_draws(ctx, D, B, shift):
    """tau = log 2, one-hot X, an offset that depends on the row's column alone (m from 0.18 to 0.82, distinct per
    column) and a weight row W[s, :] = s / 8, so that draw s sees the logit o + s / 8: column d of G[s] is the sum of r
    over the rows of column d at draw s.  Compared column by column with the reference, each column against ITS OWN
    size: a row, draw or column mix-up moves a column by a multiple of that."""
    S = 8
    X = _one_hot(B, D)
    col = np.arange(B) % D
    W = np.repeat((np.arange(S) / 8.0)[:, None], D, axis=1).astype(np.float32)
    logprec = np.full(S, math.log(2.0), np.float32)
    o = (3.0 * (col / (D - 1.0)) - 1.5).astype(np.float32)
    y = np.array([0.1, 0.3, 0.5, 0.8, 0.95], np.float32)[(np.arange(B) // D + col) % 5]
    v = (0.5 + (np.arange(B) % 4) / 4.0).astype(np.float32)
    got = _pass(ctx, X, y, W, logprec, o, v, shift=shift)
    _assert_close(got, X, y, W, logprec, o, v, what="columns")
    _, G_r, _ = ref.data_pass(X, y, W, logprec, o, v)
    # per column: the size of the float32 terms of its rows' r = v phi m (1 - m) [(ly - l1y) - psi(a) + psi(b)], each psi
    # the difference of its shifted asymptotic value (log 8 to log 9 = 2.2, hence the 5) and P' / P.  Float32 forms r to
    # about 1e-6 of that size (tests/test_glm_beta_cpu.py); 1e-5 leaves a factor 10, and a mix-up moves a column by a
    # tenth of its size or more (m changes by 0.6 across the columns, the logit by 7 / 8 across the draws).
    from scipy.special import digamma
    L = obs.logits(X, W, o)
    phi, m, m1, a, b, ly, l1y = ref._parts(L, y, logprec)
    rows = v[:, None] * phi * m * m1 * (np.abs(ly) + np.abs(l1y) + np.abs(digamma(a)) + np.abs(digamma(b)) + 5.0)
    size = np.zeros((S, D))
    for s in range(S):
        np.add.at(size[s], col, rows[:, s])
    worst = (np.abs(got[1] - G_r) / size).max()
    print("columns: worst error / size %.3g" % worst)
    assert worst <= 1e-5, worst
    assert len(set(np.round(G_r[0], 6))) > D // 2 and np.abs(G_r[0] - G_r[7]).max() > 1e-2 and np.abs(L).max() < 3.0


# ---- 4. extremes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
@pytest.mark.parametrize("flip", [1.0, -1.0])
def test_extreme_logits_through_the_offset_are_finite(ctx, D, B, flip):
    """tests/_glm_beta_ref.make_extreme_inputs: integer logits +-80 of which +-75 come from the offset (+-70 with the
    offset flipped), tau in {-2, 0, 5}, y in {1e-6, 1/4, 1/2, 1 - 1e-6}: m phi down to e^{-82} = 2.4e-36, psi(m phi) up
    to 4e35.  Everything is finite and inside the bound-based tolerances."""
    X, y, W, logprec, o, v = ref.make_extreme_inputs(D, B, flip)
    L = obs.logits(X, W, o)
    assert set(np.unique(np.abs(L[:, 0]))) == ({80.0} if flip > 0 else {70.0})
    assert (L[:, 0] > 0).any() and (L[:, 0] < 0).any() and set(logprec) == {-2.0, 0.0, 5.0}
    _check(ctx, X, y, W, logprec, o, v)


# ---- 5. zero-weight rows and the tail tile ----------------------------------------------------------------------------------

@pytest.mark.parametrize("D,shift", [(256, ()), (256, ("o",)), (64, ())])
def test_zero_weight_rows_with_wild_terms_add_exactly_nothing(ctx, D, shift):
    """35 rows, then five more of weight 0 whose y and offset are wild (0, 1, 2, NaN, 1e30; a logit of 200, -1e30, 1e30).
    35 and 40 rows make the same tiles and the same grid in both kernels, so the pass over 40 rows must return the bits
    of the pass over 35: the wild rows are dropped by a select, not multiplied away."""
    X, y, W, logprec, o, v = ref.make_inputs(40, D, 8, seed=D + 1)
    v[35:] = 0.0
    v[34] = 1.5
    y[35:] = [0.0, 1.0, 2.0, np.nan, 1.0e30]
    o[35:] = [200.0, -1.0e30, 1.0e30, 0.0, -200.0]
    a = _pass(ctx, X, y, W, logprec, o, v, shift=shift)
    b = _pass(ctx, X[:35], y[:35], W, logprec, o[:35], v[:35], shift=shift)
    for got, want, name in zip(a, b, ("ell", "G", "T")):
        assert np.isfinite(got).all(), name
        npt.assert_array_equal(got, want, err_msg=name)
    _assert_close(a, X[:35], y[:35], W, logprec, o[:35], v[:35], what="rows removed")


@pytest.mark.parametrize("D,B,shift", [(256, 13, ()), (256, 21, ()), (256, 13, ("y",)), (64, 3, ()), (8, 9, ())])
@pytest.mark.parametrize("mode", ["none", "both"])
def test_a_tail_tile_past_the_batch_forms_no_log_of_zero(ctx, mode, D, B, shift):
    """The last tile reads y = 0 past B through its descriptor (without weights nothing but the row count masks it):
    every sum is finite and the reference's."""
    X, y, W, logprec, o, v = ref.make_inputs(B, D, 8, seed=B + D, mode=mode)
    _check(ctx, X, y, W, logprec, o, v, shift=shift)


def test_two_runs_are_bit_identical(ctx):
    for B, D, S, seed in ((1029, 256, 11, 5), (165, 64, 8, 6)):
        X, y, W, logprec, o, v = ref.make_inputs(B, D, S, seed=seed)
        a = _pass(ctx, X, y, W, logprec, o, v)
        b = _pass(ctx, X, y, W, logprec, o, v)
        for p, q in zip(a, b):
            npt.assert_array_equal(p, q)


def test_an_empty_batch_gives_zeros(ctx):
    S, D = 11, 64
    W, logprec = ctx.zeros((S, D)), ctx.zeros(S)
    ell, G, T = (torch.full(s, 7.0, dtype=torch.float64, device=ctx.device) for s in ((S,), (S, D), (S,)))
    ctx.call("bsc_glm_beta_data_pass", None, D, None, None, None, 0, D, W, logprec, S, ell, G, T)
    ctx.sync()
    assert not ell.any() and not G.any() and not T.any()


# ---- 6. the finish ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S", [(256, 8), (64, 11), (8, 1)])
def test_finish_on_supplied_statistics(ctx, D, S):
    """bsc_glm_beta_update against tests/_glm_beta_ref.update on the same float64 statistics: everything is float64 on
    both sides, rtol 1e-9; the next draws are those float64 values rounded to float32.  bsc_glm_nb_update on the same
    arguments returns the same bits: the two entry points run one body."""
    f64 = torch.float64
    P = D + 1
    rs = np.random.RandomState(D + S)
    seed, t = 77, 4
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    eps, eps_n = ref.noise(D, S, seed, t - 1), ref.noise(D, S, seed, t)
    W, logprec = ref.draw(lam, eps)
    ell, G, T = 50.0 * rs.standard_normal(S), 20.0 * rs.standard_normal((S, D)), 30.0 * rs.standard_normal(S)
    m1, m2 = 0.1 * rs.standard_normal(2 * P), 0.01 * rs.uniform(size=2 * P)
    scale, prec, a0, b0, lr = 4.0, 1.5, 1.3, 0.7, 0.02
    lam_r, m1_r, m2_r, elbo_r, grad_r = ref.update(lam, m1.copy(), m2.copy(), t, eps, W, logprec, ell, G, T, scale, prec,
                                                   a0, b0, lr)

    def run(name):
        d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64),
                 m2=ctx.to_device(m2, f64), eps=ctx.to_device(eps.ravel(), f64),
                 eps_n=ctx.to_device(eps_n.ravel(), f64), W=ctx.to_device(W.ravel()), lp=_dev_vec(ctx, logprec),
                 W_n=ctx.zeros(S * D), lp_n=ctx.zeros(S), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * P, f64),
                 stats=ctx.to_device(np.concatenate([ell, G.ravel(), T]), f64))
        ctx.call(name, d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["lp"], D, S, scale, prec,
                 a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["lp_n"], d["elbo"], d["grad"])
        ctx.sync()
        return {k: a.cpu().numpy() for k, a in d.items()}

    h = run("bsc_glm_beta_update")
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

def _regression_data(B, D, seed, phi=8.0):
    """tests/test_glm_obs_gpu.py's regression data with a Beta response of precision ``phi``."""
    from scipy.special import expit
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.5 * rs.standard_normal(B) + 0.3).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    m = expit(X.astype(np.float64) @ rs.standard_normal(D) + o)
    y = np.clip(rs.beta(m * phi, (1.0 - m) * phi), ref.Y_LO, ref.Y_HI).astype(np.float32)
    return X, y, o, v


UPDATES = 10
SETUP = dict(B=2000, D=8, S=8, seed=1234, lr=0.01, prec=2.0, a0=1.5, b0=0.5, scale=10.0)


def _model(ctx, covariance, data):
    from bayesic_amd.svi import BetaReparamSVI
    c = SETUP
    X, y, o, v = data
    return BetaReparamSVI(X, y, n_total=c["scale"] * c["B"], n_samples=c["S"], seed=c["seed"], lr=c["lr"],
                          prior_precision=c["prec"], a0=c["a0"], b0=c["b0"], ctx=ctx, offset=o, weights=v,
                          covariance=covariance)


def _run_updates(ctx, covariance, check):
    """UPDATES updates of BetaReparamSVI on one batch (B = 2 000, D = 8, S = 8, offset and weights) next to the reference
    stepper of the same guide: tests/_glm_beta_ref.data_pass and the mean-field finish of tests/_glm_nb_ref.py or the
    full-covariance one of tests/_glm_scalar_full_ref.py."""
    c = SETUP
    B, D, S, P = c["B"], c["D"], c["S"], c["D"] + 1
    data = _regression_data(B, D, 10)
    X, y, o, v = data
    model = _model(ctx, covariance, data)
    is_full = covariance == "full"
    lam = full_ref.init_lam(P) if is_full else ref.init_lam(D)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    draw = full_ref.draw if is_full else ref.draw
    finish = full_ref.finish if is_full else ref.update
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, UPDATES + 1):
            assert model.step() is None
            if not check:
                continue
            eps = ref.noise(D, S, c["seed"], t - 1)
            W_r, lp_r = draw(lam, eps)
            rho = lam[full_ref.diag_slots(P)] if is_full else lam[P:]
            ell, G, T = ref.data_pass(X, y, W_r, lp_r, o, v)
            lam, m1, m2, elbo, grad = finish(lam, m1, m2, t, eps, W_r, lp_r, ell, G, T, c["scale"], c["prec"], c["a0"],
                                             c["b0"], c["lr"])
            size = ref.elbo_terms_size(W_r, lp_r, ref.bounds(X, y, W_r, lp_r, o, v)[0], c["scale"], c["prec"], c["a0"],
                                       c["b0"], rho)
            ctx.sync()
            g = model.grad.cpu().numpy()
            e = abs(model.elbo.item() - elbo)
            print("%s t=%d: ELBO %.6g, error %.3g of the terms' size %.6g; grad err/max %.3g, lam err %.3g" % (
                covariance, t, elbo, e / size, size, np.abs(g - grad).max() / np.abs(grad).max(),
                np.abs(model.lam.cpu().numpy() - lam).max()))
            assert e <= 1e-6 * size, (e, size)
            assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    ctx.sync()
    return model, lam, calls


@pytest.mark.parametrize("covariance", ["diag", "full"])
def test_several_updates_track_the_reference(ctx, covariance):
    model, lam, calls = _run_updates(ctx, covariance, check=True)
    D, P = model.D, model.D + 1
    finish = "bsc_glm_scalar_fullrank_update" if covariance == "full" else "bsc_glm_beta_update"
    assert calls.count("bsc_glm_beta_data_pass") == UPDATES and calls.count(finish) == UPDATES
    assert not [k for k in calls if (k.startswith("bsc_glm_") or k.endswith("_update")) and
                k not in ("bsc_glm_beta_data_pass", finish)]
    p = model.params()
    if covariance == "full":
        L = p["L"]
        assert L.shape == (P, P) and (np.triu(L, 1) == 0).all() and np.abs(np.tril(L, -1)).max() > 0
        npt.assert_allclose(model.covariance(), L @ L.T, rtol=1e-14)
        npt.assert_allclose(p["precision_mean"], math.exp(p["m"][D] + 0.5 * (L[D] ** 2).sum()), rtol=1e-14)
    else:
        npt.assert_array_equal(model.covariance(), np.diag(np.exp(2.0 * model.lam.cpu().numpy()[P:])))
        npt.assert_allclose(p["precision_mean"], math.exp(lam[D] + 0.5 * math.exp(2.0 * lam[2 * D + 1])), rtol=1e-3)
    assert p["tau"] == (p["m"][D], p["rho"][D]) and p["w"][0].shape == (D,)


@pytest.mark.parametrize("covariance", ["diag", "full"])
def test_two_driver_runs_from_one_seed_give_the_same_bits(ctx, covariance):
    a, _, _ = _run_updates(ctx, covariance, check=False)
    b, _, _ = _run_updates(ctx, covariance, check=False)
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    npt.assert_array_equal(a.elbo.cpu().numpy(), b.elbo.cpu().numpy())
    npt.assert_array_equal(a.grad.cpu().numpy(), b.grad.cpu().numpy())


def test_full_covariance_finish_on_the_drivers_own_statistics(ctx):
    """covariance="full" finishes through bsc_glm_scalar_fullrank_update and no kernel of this family's: three steps, and
    after each one tests/_glm_scalar_full_ref.finish fed what the DEVICE had -- lam, the Adam moments, the noise, the
    float32 draws and the statistics [ell | G | T] of the Beta pass -- gives the device's lam, gradient and ELBO at rtol
    1e-9 (float64 on both sides)."""
    c = SETUP
    D, S = c["D"], c["S"]
    model = _model(ctx, "full", _regression_data(c["B"], D, 11))
    host = lambda a: a.cpu().numpy().astype(np.float64)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 4):
            m1, m2 = host(model.m1), host(model.m2)
            model.step()
            ctx.sync()
            prev = 1 - model.cur                            # the buffers the step read
            lam_b, W_d, lp_d = host(model._lam[prev]), model._W[prev].cpu().numpy().reshape(S, D), \
                model._logprec[prev].cpu().numpy()
            eps = host(model._eps[(t - 1) % model._ring]).reshape(S, D + 1)
            npt.assert_allclose(eps, ref.noise(D, S, c["seed"], t - 1), rtol=1e-12, atol=1e-14)
            lam_r, _, _, elbo_r, grad_r = full_ref.finish(lam_b, m1, m2, t, eps, W_d, lp_d, host(model.ell),
                                                          host(model.G).reshape(S, D), host(model.T), c["scale"],
                                                          c["prec"], c["a0"], c["b0"], c["lr"])
            npt.assert_allclose(model.elbo.item(), elbo_r, rtol=1e-9)
            npt.assert_allclose(host(model.grad), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
            npt.assert_allclose(host(model.lam), lam_r, rtol=1e-9, atol=1e-12)
    finally:
        ctx.call = real_call
    assert calls.count("bsc_glm_scalar_fullrank_update") == 3 and "bsc_glm_beta_update" not in calls


def test_driver_checks_the_batch_outside_step(ctx):
    from bayesic_amd.svi import BetaReparamSVI
    B, D = 325, 64
    X, y, o, v = _regression_data(B, D, 7)
    Xd, yd, od, vd = (ctx.to_device(a) for a in (X, y, o, v))
    msg = r"strictly inside \(0, 1\) after rounding to float32"
    with pytest.raises(ValueError, match=msg):
        BetaReparamSVI(Xd, yd - yd[0], ctx=ctx)                       # one exact zero
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the Beta model takes offset="):
        BetaReparamSVI(Xd, yd, ctx=ctx, exposure=np.exp(o))
    m = BetaReparamSVI(Xd, yd, ctx=ctx, offset=od, weights=vd)
    assert m.has_offset
    for wrong in (float("nan"), 0.0, 1.0):
        bad = yd.clone()
        bad[5] = wrong
        with pytest.raises(ValueError, match=msg):
            m.set_batch(Xd, bad)
    with pytest.raises(ValueError, match="finite and >= 0"):
        m.set_batch(Xd, yd, weights=-vd - 1.0)
    m.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())   # taken as they are
    m.step()
    m2 = BetaReparamSVI(Xd, yd, ctx=ctx, offset=od, weights=vd)
    m2.step()
    ctx.sync()
    npt.assert_array_equal(m.lam.cpu().numpy(), m2.lam.cpu().numpy())
    npt.assert_array_equal(m.logprec.cpu().numpy(), m2.logprec.cpu().numpy())
    with pytest.raises(ValueError, match="fitted with an offset"):
        m2.predict(Xd, yd)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the beta model takes offset="):
        m2.predict(Xd, yd, exposure=np.exp(o))


def test_recovery_of_a_simulated_precision(ctx):
    """tests/_glm_beta_ref.recovery_data: 3 000 rows (and 500 held out) simulated at phi = 20, D = 8; 300 full-batch
    updates at S = 8, lr = 0.05 under the default priors.  precision_mean within 15 % of 20 -- the float64 reference
    alone lands at 19.89 on the same data and draws (tests/test_glm_beta_cpu.py), the device at 19.89 -- and the held-out
    log density per row beats that of the same model held at its starting point (measured: 0.81 against -0.38)."""
    from bayesic_amd.svi import BetaReparamSVI
    R = ref.RECOVERY
    X, y, w_true = ref.recovery_data(R["seed"])
    n = R["rows"]
    Xt, yt, Xh, yh = X[:n], y[:n], X[n:], y[n:]
    assert len(yh) == R["heldout"]
    kw = dict(n_samples=R["S"], seed=R["driver_seed"], lr=R["lr"], ctx=ctx)
    start = BetaReparamSVI(Xt, yt, **kw)
    lpd0 = start.heldout_lpd(Xh, yh, n_samples=64)
    model = BetaReparamSVI(Xt, yt, **kw)
    for _ in range(R["steps"]):
        model.step()
    ctx.sync()
    p = model.params()
    lpd = model.heldout_lpd(Xh, yh, n_samples=64)
    print("precision_mean %.4f; w err %.3g; held-out lpd per row %.4f (at the start %.4f)" % (
        p["precision_mean"], np.abs(p["w"][0] - w_true).max(), lpd, lpd0))
    assert abs(p["precision_mean"] - 20.0) <= 0.15 * 20.0
    assert math.isfinite(lpd) and math.isfinite(lpd0) and lpd > lpd0


# ---- 8. the predictive ------------------------------------------------------------------------------------------------------

def _predict(ctx, X, y, W, logprec, o, shift=False, want=("mean", "var", "lpd", "lpd_sum")):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od, pd = _dev_vec(ctx, y), _dev_vec(ctx, o, shift), _dev_vec(ctx, logprec, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in ("mean", "var", "lpd", "lpd_sum")]
    ctx.call("bsc_beta_predict_pass", Xd, D, yd, od, B, D, Wd, pd, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, X, y, W, logprec, o, v=None, keys=("mean", "var", "lpd", "lpd_sum")):
    want = ref.predict(X, W, logprec, y, o, v)
    bnd = ref.predict_bounds(X, W, logprec, y, o, v)
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        print("beta %s: worst error / bound %.3g" % (k, worst))
        assert worst <= 1.0, (k, worst)


def _predict_inputs(B, D, S, seed, offset=True):
    X, y, W, logprec, o, _ = ref.make_inputs(B, D, S, seed, mode="offset")
    return X, y, W, logprec, (o if offset else None)


@pytest.mark.parametrize("B,D,S,shift,offset", [(1, 8, 1, False, True), (17, 8, 16, False, False),
                                                (17, 8, 33, True, True), (1029, 8, 64, False, True),
                                                (17, 252, 1, True, True), (1029, 252, 16, False, False),
                                                (1, 252, 33, False, True), (17, 252, 64, False, True),
                                                (17, 256, 1, True, True), (1029, 256, 16, False, False),
                                                (1, 256, 33, False, True), (1029, 256, 64, True, True)])
def test_predict_matches_the_reference(ctx, B, D, S, shift, offset):
    X, y, W, logprec, o = _predict_inputs(B, D, S, B + D + S, offset)
    got = _predict(ctx, X, y, W, logprec, o, shift=shift)
    _assert_predict(got, X, y, W, logprec, o)


def test_predict_optional_outputs_and_no_response(ctx):
    X, y, W, logprec, o = _predict_inputs(165, 64, 16, 9)
    full = _predict(ctx, X, y, W, logprec, o)
    for want in (("mean",), ("var",), ("lpd",), ("lpd_sum",), ("mean", "lpd_sum")):
        got = _predict(ctx, X, y, W, logprec, o, want=want)
        for k in ("mean", "var", "lpd", "lpd_sum"):
            if k in want:
                npt.assert_array_equal(got[k], full[k], err_msg=k)
            else:
                assert (got[k] == -777.0).all(), k
    # without y: the moments alone
    B, D = X.shape
    mean = torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device)
    var = torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device)
    ctx.call("bsc_beta_predict_pass", ctx.to_device(X), D, None, _dev_vec(ctx, o), B, D, ctx.to_device(W),
             _dev_vec(ctx, logprec), 16, mean, var, None, None)
    ctx.sync()
    npt.assert_array_equal(mean.cpu().numpy(), full["mean"])
    npt.assert_array_equal(var.cpu().numpy(), full["var"])


def test_predict_several_tiles_per_wave_pairs_every_row_with_its_offset(ctx, cu):
    B = 8 * cu * 16 + 16 + 5
    rs = np.random.RandomState(2)
    X = (rs.standard_normal((B, 256)) / 16.0).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, 256))).astype(np.float32)
    logprec = np.linspace(ref.TAU_LO, ref.TAU_HI, 8).astype(np.float32)
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)
    y = np.array([ref.Y_LO, 0.01, 0.2, 0.5, 0.7, 0.97, ref.Y_HI], np.float32)[np.arange(B) % 7]
    got = _predict(ctx, X, y, W, logprec, o)
    _assert_predict(got, X, y, W, logprec, o)


def test_driver_predict_with_offset_and_weights(ctx):
    from bayesic_amd.svi import BetaReparamSVI
    from bayesic_amd.svi import predict as mod
    B, D = 600, 8
    X, y, o, _ = _regression_data(B, D, 12)
    m = BetaReparamSVI(X, y, offset=o, n_samples=8, seed=9, lr=0.05, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    assert mod.family_of(m) == "beta"
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    draws = mod.posterior_draws(m, 16)
    W, logprec = draws[0].cpu().numpy(), draws[1].cpu().numpy()
    W_r, lp_r = ref.posterior_draws(m.lam.cpu().numpy(), D, 16, m.seed)             # Philox stream 2
    npt.assert_array_equal(W, W_r)
    npt.assert_array_equal(logprec, lp_r)
    out = m.predict(X, y, offset=o, draws=draws)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _assert_predict(got, X, y, W, logprec, o)
    assert m.heldout_lpd(X, y, offset=o, draws=draws) == float(out["lpd_sum"].item()) / B
    none = m.predict(X, None, offset=o, draws=draws)                               # y=None: the moments alone
    assert sorted(none) == ["mean", "var"]
    npt.assert_array_equal(none["mean"].cpu().numpy(), got["mean"])
    npt.assert_array_equal(none["var"].cpu().numpy(), got["var"])
    v = np.random.RandomState(3).uniform(0.0, 2.0, B).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, offset=o, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, X, y, W, logprec, o, v)
    score = m.heldout_lpd(X, y, offset=o, weights=v, draws=draws)
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())
    assert float(wout["weight_sum"].item()) == float(v.astype(np.float64).sum())
    # a model fitted without an offset predicts without one
    m0 = BetaReparamSVI(X, y, n_samples=8, seed=9, ctx=ctx)
    m0.step()
    d0 = mod.posterior_draws(m0, 33)
    g0 = {k: t.cpu().numpy() for k, t in m0.predict(X, y, draws=d0).items()}
    _assert_predict(g0, X, y, d0[0].cpu().numpy(), d0[1].cpu().numpy(), None)


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9) + 0.5, ctx.zeros((65, 260))
    o, v, lp = ctx.zeros(12), ctx.zeros(12), ctx.zeros(68)
    ell, G, T = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros(65, f64)

    def call(Xa, ldx, D, S, Wa=W, pa=lp, ya=y, B=8, oa=o, va=v):
        ctx.call("bsc_glm_beta_data_pass", Xa, ldx, ya, oa, va, B, D, Wa, pa, S, ell, G, T)

    for kw, match in ((dict(Xa=X, ldx=8, D=6, S=8), "D=6 must be a multiple of 4"),
                      (dict(Xa=X, ldx=260, D=260, S=8), "D=260 must be a multiple of 4 in"),
                      (dict(Xa=X, ldx=256, D=256, S=65), "S=65"),
                      (dict(Xa=X.view(-1)[1:], ldx=256, D=256, S=8), "X and W must be 16-byte aligned"),
                      (dict(Xa=X, ldx=6, D=8, S=8), "ldx=6"),
                      (dict(Xa=X, ldx=256, D=256, S=8, pa=None), "logprec is null"),
                      (dict(Xa=X, ldx=256, D=256, S=8, pa=lp.data_ptr() + 2), "logprec must be 4-byte aligned"),
                      (dict(Xa=X, ldx=256, D=256, S=8, ya=None), "y is null with B=8")):
        with pytest.raises(BayesicHipError, match="bsc_glm_beta_data_pass: " + match):
            call(**kw)
    with pytest.raises(BayesicHipError, match="bsc_glm_beta_data_pass: null output"):
        ctx.call("bsc_glm_beta_data_pass", X, 256, y, o, v, 8, 256, W, lp, 8, ell, G, None)

    lam, m = ctx.zeros((2, 18), f64), ctx.zeros((2, 18), f64)
    eps = ctx.zeros((2, 8 * 9), f64)
    stats = ctx.zeros(8 * 10, f64)
    Wn, pn = ctx.zeros(8 * 8), ctx.zeros(8)

    def update(st=stats, S=8, a0=1.0, b0=1.0, t=1, p=lp):
        ctx.call("bsc_glm_beta_update", st, lam[0], lam[1], m[0], m[1], eps[0], W, p, 8, S, 1.0, 1.0, a0, b0, t, 0.01,
                 0.9, 0.999, 1e-8, 1, 1, eps[1], 1, Wn, pn, ell, G)

    with pytest.raises(BayesicHipError, match="bsc_glm_beta_update: stats is null"):
        update(st=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_beta_update: null pointer"):
        update(p=None)
    with pytest.raises(BayesicHipError, match="bsc_glm_beta_update: a0=0 b0=1 must be positive"):
        update(a0=0.0)
    with pytest.raises(BayesicHipError, match=r"bsc_glm_beta_update: D=8 S=65 \(S<=64\)"):
        update(S=65)
    with pytest.raises(BayesicHipError, match="bsc_glm_beta_update: the Adam step count starts at 1"):
        update(t=0)

    out = ctx.zeros(9)

    def predict(D=8, S=8, Xa=X, ya=y, pa=lp, ldx=8, outs=(out, None, None, None)):
        ctx.call("bsc_beta_predict_pass", Xa, ldx, ya, o, 8, D, W, pa, S, *outs)

    with pytest.raises(BayesicHipError, match="bsc_beta_predict_pass: logprec is null"):
        predict(pa=None)
    with pytest.raises(BayesicHipError, match="bsc_beta_predict_pass: offset and logprec must be 4-byte aligned"):
        predict(pa=lp.data_ptr() + 2)
    with pytest.raises(BayesicHipError, match="bsc_beta_predict_pass: lpd and lpd_sum need y"):
        predict(ya=None, outs=(None, None, out, None))
    with pytest.raises(BayesicHipError, match="bsc_beta_predict_pass: no output requested"):
        predict(outs=(None, None, None, None))
    for kw, match in ((dict(S=65), "bsc_beta_predict_pass: S=65"),
                      (dict(D=6), "bsc_beta_predict_pass: D=6 must be a multiple of 4")):
        with pytest.raises(BayesicHipError, match=match) as err:
            predict(**kw)
        assert "status -3:" in str(err.value), str(err.value)          # BSC_ERR_UNSUPPORTED
    ctx.sync()


