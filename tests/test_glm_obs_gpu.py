"""GPU parity of the GLM route with per-row offsets, exposure and weights (csrc/bsc_glm_obs.hip and
csrc/bsc_predict_offset.hip through the C ABI, svi/glm.py, svi/predict.py) against the float64 restatement in
tests/_glm_obs_ref.py.

Tolerances are tests/test_glm_gpu.py's with the bound quantity weighted:
 * ell: |dev - ref| <= 2e-5 * sum_n v_n (|y_n l_ns| + A(l_ns) + 1), l including the offset, rows of weight 0 left out;
 * G: rtol 1e-4, atol 1e-4 * max|G|;
 * exact-integer layouts: ell rtol 1e-6, G rtol 1e-6 (atol 2e-7 for the logistic link); extreme logits rtol 1e-6;
 * several updates against the reference: ELBO rtol 1e-6, gradient 1e-4 * max|grad|, lam atol 2e-4 (full guide: ELBO
   rtol 1e-6, lam atol 1e-4, tests/test_glm_full_gpu.py's);
 * the predictive: tests/test_predict_gpu.py's bounds with a_ns = sum_d |x_nd w_sd| + |o_n| (tests/_glm_obs_ref.py).
Poisson inputs keep |l| <= 4 including the offset, except where a test is about a wild link value.

Shapes are the smallest that reach each path: B in {1, 7, 37, 16 k + 5}, D in {8, 64, 252, 256}, S in {1, 8, 11}
(11 = two launches), ldx > D; at D = 256 the 16-row MFMA kernel with every vector 16-byte aligned and the 8-row kernel
with each of y, o, v four bytes into its buffer; and batches sized from the device's CU count for 2 and 3 tiles per
wave, where the offsets and weights of the prefetched tile and the current one have to be kept apart."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_full_ref as full_ref
import _glm_obs_ref as ref
import _glm_ref as glm
import _predict_ref as pred

pytestmark = pytest.mark.gpu

LINKS = ("logistic", "poisson")
CODE = {"logistic": 0, "poisson": 1}
MODES = ("offset", "weights", "both")
SENTINEL = 1.0e30      # behind the end of y / o / v: a read past B would wreck the sums


def _dev_vec(ctx, a, shift=False, guard=16):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[SENTINEL] if shift else [], a, np.full(guard, SENTINEL)]).astype(np.float32)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _pass(ctx, link, X, y, W, o=None, v=None, ld=None, shift=(), name="bsc_glm_data_pass_obs"):
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
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    if name == "bsc_glm_data_pass":
        ctx.call(name, CODE[link], Xd, (ld or D), yd, B, D, Wd, S, ell, G)
    else:
        ctx.call(name, CODE[link], Xd, (ld or D), yd, od, vd, B, D, Wd, S, ell, G)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy()


def _inputs(link, B, D, S, seed, mode="both"):
    """test_glm_gpu._inputs' recipe with offsets N(0, 1) and weights U(0, 3), every fifth weight exactly zero."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    if link == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, W, o)).max() if B else 0.0
        if peak > 3.5:
            W, o = (W * (3.5 / peak)).astype(np.float32), (o * (3.5 / peak)).astype(np.float32)
    return X, y, W, (o if mode != "weights" else None), (v if mode != "offset" else None)


def _assert_close(link, got, X, y, W, o, v, what=""):
    ell, G = got
    ell_r, G_r = ref.data_pass(link, X, y, W, o, v)
    bound = ref.ell_bound(link, X, y, W, o, v)
    err = np.abs(ell - ell_r)
    print("%s %s B=%d D=%d S=%d: ell err/bound %.3g, G err/max %.3g" % (
        what, link, X.shape[0], X.shape[1], W.shape[0], (err / (bound + 1e-300)).max(),
        np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300)))
    assert (err <= 2e-5 * bound + 1e-12).all(), (err / (bound + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())


def _check(ctx, link, X, y, W, o, v, **kw):
    if link == "poisson":
        assert np.abs(ref.logits(X, W, o)).max() <= 4.0
    got = _pass(ctx, link, X, y, W, o, v, **kw)
    _assert_close(link, got, X, y, W, o, v)
    return got


# ---- parity over the envelope ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S,ld", [(1, 8, 1, None), (7, 8, 8, 12), (37, 64, 11, None), (53, 64, 8, 96),
                                      (7, 252, 8, None), (165, 252, 11, 256), (1, 256, 8, None), (7, 256, 1, None),
                                      (37, 256, 8, 260), (325, 256, 11, None), (1029, 256, 8, 512)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("link", LINKS)
def test_pass_matches_the_reference(ctx, link, mode, B, D, S, ld):
    X, y, W, o, v = _inputs(link, B, D, S, seed=B * 7 + D + S, mode=mode)
    _check(ctx, link, X, y, W, o, v, ld=ld)


@pytest.mark.parametrize("shift", [(), ("y",), ("o",), ("v",), ("y", "o", "v")])
@pytest.mark.parametrize("link", LINKS)
def test_full_width_with_aligned_and_misaligned_vectors(ctx, link, shift):
    """D = 256: every vector 16-byte aligned takes the 16-row MFMA kernel, any one four bytes in the 8-row kernel (the
    MFMA kernel loads y, o and v sixteen bytes at a time).  Both must agree with the reference -- and with each other
    within the two bounds, which they would not if a misaligned vector were read sixteen bytes at a time."""
    X, y, W, o, v = _inputs(link, 1003, 256, 8, seed=3)
    _check(ctx, link, X, y, W, o, v, shift=shift)


# ---- several tiles per wave -----------------------------------------------------------------------------------------

def _grid(B, rows, cu):
    n_tiles = (B + rows - 1) // rows
    max_waves = 8 * cu
    n_iter = (n_tiles + max_waves - 1) // max_waves
    return n_iter


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


@pytest.mark.parametrize("kernel,D,n_iter", [("mfma", 256, 2), ("mfma", 256, 3), ("valu", 256, 2), ("valu", 64, 3),
                                             ("valu", 252, 2)])
@pytest.mark.parametrize("link", LINKS)
def test_several_tiles_per_wave_keep_each_rows_offset_and_weight(ctx, cu, link, kernel, D, n_iter):
    """B = (n_iter - 1) sweeps of the resident waves + one tile + 5 rows (tests/test_regression_multi_tile_gpu.py's
    form).  Every row has its own offset and weight, so a tile computed with the prefetched tile's o or v -- the
    hand-over these kernels add -- moves ell and G far outside the bounds; sentinels of 1e30 sit behind y, o and v."""
    rows = 16 if kernel == "mfma" else 8
    B = (n_iter - 1) * 8 * cu * rows + rows + 5
    assert _grid(B, rows, cu) == n_iter
    rs = np.random.RandomState(n_iter + D)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, D))).astype(np.float32)
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)          # distinct within any two tiles of a wave
    v = (0.25 + (np.arange(B) % 1013) / 500.0).astype(np.float32)
    v[::7] = 0.0
    y = ((np.arange(B) % 3) == 0).astype(np.float32) if link == "logistic" else (np.arange(B) % 4).astype(np.float32)
    shift = ("y",) if (kernel == "valu" and D == 256) else ()
    _check(ctx, link, X, y, W, o, v, shift=shift)


# ---- exact layout ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,shift", [(256, ()), (256, ("v",)), (64, ())])
@pytest.mark.parametrize("link", LINKS)
def test_row_to_offset_and_weight_mapping_with_exact_integers(ctx, link, D, shift):
    """W = 0 and one-hot X (row n has its 1 in column n): l[n, s] = o_n, column n of G is v_n (y_n - A'(o_n)) for every
    draw, and ell[s] = sum_n v_n (y_n o_n - A(o_n)).  Offsets are small integers, weights powers of two (1, 1/2, 1/4:
    exact products that do not enlarge the absolute error of 1 - sigmoid the existing atol stands for), so any mix-up
    of the row -> (o, v) mapping in either kernel shows at the existing exact-integer bounds."""
    B, S = (D, 8) if D == 64 else (200, 8)
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B)] = 1.0
    W = np.zeros((S, D), np.float32)
    o = ((np.arange(B) * 5) % 7 - 3).astype(np.float32)
    v = (2.0 ** -((np.arange(B) * 2) % 3)).astype(np.float32)
    v[::11] = 0.0
    y = (np.arange(B) % 3 == 0).astype(np.float32)
    ell, G = _pass(ctx, link, X, y, W, o, v, shift=shift)
    ell_r, G_r = ref.data_pass(link, X, y, W, o, v)
    npt.assert_allclose(ell, ell_r, rtol=1e-6)
    npt.assert_allclose(G, G_r, rtol=1e-6, atol=2e-7 if link == "logistic" else 0.0)
    assert len(set(np.round(G_r[0], 5))) > 12


@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
def test_logistic_at_extreme_logits_through_the_offset(ctx, D, B):
    """Total logits +-80 of which +-75 come from the offset."""
    S = 8
    X = np.zeros((B, D), np.float32)
    X[np.arange(B), np.arange(B) % D] = 1.0
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(D)[None, :])
    W = (5.0 * sign).astype(np.float32)
    y = ((np.arange(B) // 2) % 2).astype(np.float32)
    v = (1.0 + (np.arange(B) % 3)).astype(np.float32)
    for flip in (1.0, -1.0):
        # draw 0 sees l = +-5 +- 75 = +-80 on every row; the other draws +-80 or +-70
        o = (flip * 75.0 * sign[0, np.arange(B) % D]).astype(np.float32)
        L = ref.logits(X, W, o)
        assert set(np.unique(np.abs(L[:, 0]))) == ({80.0} if flip > 0 else {70.0})
        ell, G = _pass(ctx, "logistic", X, y, W, o, v)
        assert np.isfinite(ell).all() and np.isfinite(G).all()
        ell_r, G_r = ref.data_pass("logistic", X, y, W, o, v)
        npt.assert_allclose(ell, ell_r, rtol=1e-6)
        npt.assert_allclose(G, G_r, rtol=1e-6)


@pytest.mark.parametrize("D,shift", [(256, ()), (256, ("o",)), (64, ())])
def test_zero_weight_rows_with_wild_link_values_are_neutral(ctx, D, shift):
    """Poisson rows with a total logit of 200 (exp overflows float32) and weight 0: ell and G stay finite and equal the
    pass over the batch without those rows, each within its bound.  Without weights the same rows give a non-finite
    result -- an ordinary numerical outcome of exp(200), no fault."""
    link, B = "poisson", 165
    X, y, W, o, v = _inputs(link, B, D, 8, seed=D)
    wild = np.array([0, 17, 33, 164])
    o[wild] = 200.0
    v[wild] = 0.0
    got = _pass(ctx, link, X, y, W, o, v, shift=shift)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    keep = np.ones(B, bool)
    keep[wild] = False
    _assert_close(link, got, X[keep], y[keep], W, o[keep], v[keep], what="rows removed")
    ell, G = _pass(ctx, link, X, y, W, o, None, shift=shift)
    assert not np.isfinite(ell).all() and not np.isfinite(G).all()


# ---- identities on the device ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [256, 64])
def test_binomial_rows_against_their_expansion(ctx, D):
    """(x, y = k / n, v = n) against the n Bernoulli rows through the pass without weights: each within its own bound
    of the float64 reference, which agree with each other (tests/test_glm_obs_cpu.py)."""
    rs = np.random.RandomState(D)
    B = 85
    X, _, W, o, _ = _inputs("logistic", B, D, 8, seed=D + 1)
    n = rs.randint(1, 9, B)
    k = rs.binomial(n, 0.4)
    yk = (k / n).astype(np.float32)
    _check(ctx, "logistic", X, yk, W, o, n.astype(np.float32))
    Xe, ye = ref.expand_binomial(X, k, n)
    oe = np.repeat(o, n)
    got_e = _pass(ctx, "logistic", Xe, ye, W, oe, None)
    _assert_close("logistic", got_e, Xe, ye, W, oe, None, what="expanded")
    agg = ref.data_pass("logistic", X, yk, W, o, n.astype(np.float32))
    exp_ = ref.data_pass("logistic", Xe, ye, W, oe, None)
    npt.assert_allclose(agg[0], exp_[0], rtol=1e-6)          # y = k / n rounded to float32
    npt.assert_allclose(agg[1], exp_[1], rtol=1e-5, atol=1e-6 * np.abs(exp_[1]).max())


@pytest.mark.parametrize("D", [8, 64, 252])
@pytest.mark.parametrize("link", LINKS)
def test_offset_as_a_column_of_the_shipped_pass(ctx, link, D):
    """The obs pass on (X, o) against bsc_glm_data_pass on [X | o 0 0 0] with W' = [W | 1 0 0 0]: ell and G[:, :D],
    each within its bound of the same float64 reference."""
    B, S = 165, 8
    X, y, W, o, _ = _inputs(link, B, D, S, seed=D, mode="offset")
    got = _check(ctx, link, X, y, W, o, None)
    X2 = np.zeros((B, D + 4), np.float32)
    X2[:, :D], X2[:, D] = X, o
    W2 = np.zeros((S, D + 4), np.float32)
    W2[:, :D], W2[:, D] = W, 1.0
    ell2, G2 = _pass(ctx, link, X2, y, W2, name="bsc_glm_data_pass")
    _assert_close(link, (ell2, G2[:, :D]), X, y, W, o, None, what="as a column")
    bound = ref.ell_bound(link, X, y, W, o, None)
    assert (np.abs(got[0] - ell2) <= 2 * 2e-5 * bound).all()


# ---- bit-for-bit equalities -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D,S", [(325, 256, 11), (165, 64, 8)])
@pytest.mark.parametrize("link", LINKS)
def test_without_offset_and_weight_it_is_the_shipped_pass_bit_for_bit(ctx, link, B, D, S):
    X, y, W, _, _ = _inputs(link, B, D, S, seed=9)
    a = _pass(ctx, link, X, y, W, name="bsc_glm_data_pass")
    b = _pass(ctx, link, X, y, W, None, None)
    npt.assert_array_equal(a[0], b[0])
    npt.assert_array_equal(a[1], b[1])


@pytest.mark.parametrize("link", LINKS)
def test_two_runs_are_bit_identical(ctx, link):
    X, y, W, o, v = _inputs(link, 1029, 256, 11, seed=5)
    a = _pass(ctx, link, X, y, W, o, v)
    b = _pass(ctx, link, X, y, W, o, v)
    npt.assert_array_equal(a[0], b[0])
    npt.assert_array_equal(a[1], b[1])


def _update_state(ctx, D, S, seed, t):
    rs = np.random.RandomState(D + S)
    f64 = torch.float64
    lam = np.concatenate([0.2 * rs.standard_normal(D), math.log(0.1) + 0.1 * rs.standard_normal(D)])
    eps = np.zeros((S, D + 1))
    eps[:, :D] = glm.noise(D, S, seed, t - 1)
    eps_n = np.zeros((S, D + 1))
    eps_n[:, :D] = glm.noise(D, S, seed, t)
    W = glm.draw(lam, eps[:, :D])
    d = dict(lam=ctx.to_device(lam, f64), out=ctx.zeros(2 * D, f64), m1=ctx.zeros(2 * D, f64), m2=ctx.zeros(2 * D, f64),
             eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()), eps_n=ctx.to_device(eps_n.ravel(), f64),
             W_n=ctx.zeros(S * D), elbo=ctx.zeros(1, f64), grad=ctx.zeros(2 * D, f64))
    return d, W


@pytest.mark.parametrize("D,both", [(256, True), (64, True), (64, False)])
@pytest.mark.parametrize("link", LINKS)
def test_one_call_update_equals_pass_then_update(ctx, link, D, both):
    """bsc_glm_pass_update_obs against bsc_glm_data_pass_obs -> bsc_glm_update(stats); with both vectors NULL also
    against bsc_glm_pass_update.  The one-call form sums the slab inside the finish, the other through the float64
    reduction kernel: the same partials in the same order, so lam, the moments, ELBO and gradient agree bit for bit."""
    B, S, seed, t = 325, 8, 31, 3
    X, y, _, o, v = _inputs(link, B, D, S, seed=D + 2)
    if not both:
        o = v = None
    scale, tau, lr = 4.0, 1.5, 0.02
    outs = []
    names = ["bsc_glm_pass_update_obs", "two calls"] + ([] if both else ["bsc_glm_pass_update"])
    Xd, yd, od, vd = ctx.to_device(X), ctx.to_device(y), _dev_vec(ctx, o), _dev_vec(ctx, v)
    for name in names:
        d, W = _update_state(ctx, D, S, seed, t)
        tail = (scale, tau, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], 1, d["W_n"], d["elbo"], d["grad"])
        state = (d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], S)
        if name == "bsc_glm_pass_update_obs":
            ctx.call(name, CODE[link], Xd, D, yd, od, vd, B, D, *state, *tail)
        elif name == "bsc_glm_pass_update":
            ctx.call(name, CODE[link], Xd, D, yd, B, D, *state, *tail)
        else:
            stats = ctx.zeros(S * (D + 1), torch.float64)
            ctx.call("bsc_glm_data_pass_obs", CODE[link], Xd, D, yd, od, vd, B, D, d["W"], S, stats[:S], stats[S:])
            ctx.call("bsc_glm_update", stats, d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], D, S, *tail)
        ctx.sync()
        outs.append({k: d[k].cpu().numpy().copy() for k in ("out", "m1", "m2", "elbo", "grad", "W_n")})
    for other in outs[1:]:
        for k, a in outs[0].items():
            npt.assert_array_equal(a, other[k], err_msg=k)
    assert np.abs(outs[0]["out"]).max() > 0 and np.isfinite(outs[0]["elbo"]).all()


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9), ctx.zeros((65, 260))
    o, v = ctx.zeros(12), ctx.zeros(12)
    ell, G = ctx.zeros(65, torch.float64), ctx.zeros((65, 260), torch.float64)

    def call(link, Xa, ldx, D, S, ya=y, B=8):
        ctx.call("bsc_glm_data_pass_obs", link, Xa, ldx, ya, o, v, B, D, W, S, ell, G)

    with pytest.raises(BayesicHipError, match="bsc_glm_data_pass_obs: y is null with B=8"):
        call(0, X, 256, 256, 8, ya=None)
    # the envelope of the shipped pass, unchanged through the new entry point
    with pytest.raises(BayesicHipError, match="bsc_glm_data_pass_obs: D=6 must be a multiple of 4"):
        call(0, X, 8, 6, 8)
    with pytest.raises(BayesicHipError, match="D=260 must be a multiple of 4 in"):
        call(0, X, 260, 260, 8)
    with pytest.raises(BayesicHipError, match="16-byte aligned"):
        call(0, X.view(-1)[1:], 256, 256, 8)
    with pytest.raises(BayesicHipError, match="S=65"):
        call(1, X, 256, 256, 65)
    with pytest.raises(BayesicHipError, match="link=2"):
        call(2, X, 256, 256, 8)
    with pytest.raises(BayesicHipError, match="ldx=6"):
        call(0, X, 6, 8, 8)
    lam, m = ctx.zeros((2, 16), torch.float64), ctx.zeros((2, 16), torch.float64)
    eps = ctx.zeros((2, 8 * 9), torch.float64)
    with pytest.raises(BayesicHipError, match="bsc_glm_pass_update_obs: S=9"):
        ctx.call("bsc_glm_pass_update_obs", 0, X, 8, y, o, v, 8, 8, lam[0], lam[1], m[0], m[1], eps[0], W, 9, 1.0, 1.0,
                 1, 0.01, 0.9, 0.999, 1e-8, 1, 1, eps[1], 1, W, ell, G)
    out = ctx.zeros(9)
    with pytest.raises(BayesicHipError, match="bsc_predict_pass_offset: offset is for .* the Gaussian family"):
        ctx.call("bsc_predict_pass_offset", 0, X, 8, y, o, 8, 8, W, ctx.zeros(8), 8, out, None, None, None)
    with pytest.raises(BayesicHipError, match="bsc_predict_pass_offset: lpd and lpd_sum need y"):
        ctx.call("bsc_predict_pass_offset", 2, X, 8, None, o, 8, 8, W, None, 8, None, None, out, None)
    with pytest.raises(BayesicHipError, match="bsc_predict_pass_offset: S=65"):
        ctx.call("bsc_predict_pass_offset", 1, X, 8, y, o, 8, 8, W, None, 65, out, None, None, None)
    ctx.sync()


# ---- the predictive -------------------------------------------------------------------------------------------------

def _predict(ctx, family, X, y, W, o, name="bsc_predict_pass_offset", shift=False):
    B, D = X.shape
    S = W.shape[0]
    Xd, Wd = ctx.to_device(X), ctx.to_device(W)
    yd, od = _dev_vec(ctx, y), _dev_vec(ctx, o, shift)
    out = {k: torch.full((B,), -777.0, dtype=torch.float32, device=ctx.device) for k in ("mean", "var", "lpd")}
    out["lpd_sum"] = torch.full((1,), -777.0, dtype=torch.float64, device=ctx.device)
    args = [out[k] for k in ("mean", "var", "lpd", "lpd_sum")]
    if name == "bsc_predict_pass":
        ctx.call(name, pred.CODE[family], Xd, D, yd, B, D, Wd, None, S, *args)
    else:
        ctx.call(name, pred.CODE[family], Xd, D, yd, od, B, D, Wd, None, S, *args)
    ctx.sync()
    return {k: t.cpu().numpy() for k, t in out.items()}


def _assert_predict(got, family, X, y, W, o, v=None):
    want = ref.predict(family, X, W, y, o, v)
    bnd = ref.predict_bounds(family, X, W, y, o, v)
    for k in ("mean", "var", "lpd", "lpd_sum"):
        worst = float(np.max(np.abs(got[k] - want[k]) / (bnd[k] + 1e-300)))
        print("%s %s: worst error / bound %.3g" % (family, k, worst))
        assert worst <= 1.0, (k, worst)


@pytest.mark.parametrize("B,D,S,shift", [(1, 8, 1, False), (37, 64, 24, False), (165, 252, 8, True),
                                         (1003, 256, 8, False), (1003, 256, 64, True), (53, 64, 40, False)])
@pytest.mark.parametrize("family", LINKS)
def test_predict_with_an_offset_matches_the_reference(ctx, family, B, D, S, shift):
    X, y, W, o, _ = _inputs(family, B, D, S, seed=B + D + S, mode="offset")
    got = _predict(ctx, family, X, y, W, o, shift=shift)
    _assert_predict(got, family, X, y, W, o)


@pytest.mark.parametrize("family", LINKS)
def test_predict_several_tiles_per_wave_pairs_every_row_with_its_offset(ctx, cu, family):
    """Two tiles per wave at D = 256 (8 waves on each CU): the offset of the next tile is fetched while the current one
    is still to be used."""
    B = 8 * cu * 16 + 16 + 5
    rs = np.random.RandomState(2)
    X = (rs.standard_normal((B, 256)) / 16.0).astype(np.float32)
    W = (0.4 * rs.standard_normal((8, 256))).astype(np.float32)
    o = (0.002 * (np.arange(B) % 997) - 1.0).astype(np.float32)
    y = (np.arange(B) % 2).astype(np.float32)
    got = _predict(ctx, family, X, y, W, o)
    _assert_predict(got, family, X, y, W, o)


@pytest.mark.parametrize("family", LINKS)
def test_predict_without_an_offset_is_the_shipped_pass_bit_for_bit(ctx, family):
    X, y, W, _, _ = _inputs(family, 1003, 256, 24, seed=4)
    a = _predict(ctx, family, X, y, W, None, name="bsc_predict_pass")
    b = _predict(ctx, family, X, y, W, None)
    c = _predict(ctx, family, X, y, W, np.zeros(1003, np.float32))
    for k in a:
        npt.assert_array_equal(a[k], b[k], err_msg=k)
    _assert_predict(c, family, X, y, W, None)


def _count_model(ctx, B=600, D=8, steps=3, **kw):
    from bayesic_amd.svi import GLMReparamSVI
    rs = np.random.RandomState(12)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    expo = np.exp(rs.uniform(math.log(0.1), math.log(10.0), B)).astype(np.float32)
    y = rs.poisson(expo * np.exp(X.astype(np.float64) @ (0.5 * rs.standard_normal(D)))).astype(np.float32)
    m = GLMReparamSVI(X, y, link="poisson", exposure=expo, n_samples=8, seed=9, lr=0.05, ctx=ctx, **kw)
    for _ in range(steps):
        m.step()
    ctx.sync()
    return m, X, y, expo


def test_driver_predict_with_exposure_and_weights(ctx):
    from bayesic_amd.svi import predict as mod
    m, X, y, expo = _count_model(ctx)
    assert m.has_offset
    npt.assert_allclose(m.offset.cpu().numpy(), np.log(expo.astype(np.float64)), rtol=2e-7, atol=1e-7)   # one float32 log
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y)
    draws = mod.posterior_draws(m, 16)
    W = draws[0].cpu().numpy()
    o = m.offset.cpu().numpy()
    out = m.predict(X, y, exposure=expo, draws=draws)
    got = {k: t.cpu().numpy() for k, t in out.items()}
    _assert_predict(got, "poisson", X, y, W, o)
    # the same through offset=, bit for bit
    out_o = m.predict(X, y, offset=o, draws=draws)
    for k in got:
        npt.assert_array_equal(out_o[k].cpu().numpy(), got[k])
    # doubling the exposure doubles the mean to float32 rounding: on either side log(exposure), l + o and the argument
    # of exp are rounded at magnitudes <= 8 (half an ulp, 4.8e-7, each) and expf adds two ulps: 2 (3 * 4.8e-7 + 2.4e-7)
    twice = m.predict(X, exposure=2.0 * expo, draws=draws)["mean"].cpu().numpy()
    assert np.abs(ref.logits(X, W, o)).max() + math.log(2.0) <= 8.0
    npt.assert_allclose(twice, 2.0 * got["mean"], rtol=3.4e-6)
    # weights: lpd per row is untouched, lpd_sum and the held-out score are weighted
    v = np.random.RandomState(3).uniform(0.0, 2.0, X.shape[0]).astype(np.float32)
    v[::4] = 0.0
    wout = m.predict(X, y, exposure=expo, weights=v, draws=draws)
    wgot = {k: wout[k].cpu().numpy() for k in ("mean", "var", "lpd", "lpd_sum")}
    npt.assert_array_equal(wgot["lpd"], got["lpd"])
    _assert_predict(wgot, "poisson", X, y, W, o, v)
    score = m.heldout_lpd(X, y, exposure=expo, weights=v, draws=draws)
    want = ref.predict("poisson", X, W, y, o, v)["lpd_sum"] / v.astype(np.float64).sum()
    bound = ref.predict_bounds("poisson", X, W, y, o, v)["lpd_sum"] / v.astype(np.float64).sum()
    assert abs(score - want) <= bound
    assert score == float(wout["lpd_sum"].item()) / float(wout["weight_sum"].item())


# ---- drivers --------------------------------------------------------------------------------------------------------

def _regression_data(link, B, D, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    o = (0.5 * rs.standard_normal(B)).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    L = X.astype(np.float64) @ rs.standard_normal(D) + o
    if link == "logistic":
        y = (rs.uniform(size=B) < 1.0 / (1.0 + np.exp(-L))).astype(np.float32)
    else:
        y = rs.poisson(np.exp(L)).astype(np.float32)
    return X, y, o, v


@pytest.mark.parametrize("S", [8, 11])            # the one-call path / data pass -> all-reduce -> finish(stats)
@pytest.mark.parametrize("link", LINKS)
def test_twenty_updates_track_the_reference_over_two_batches(ctx, link, S):
    from bayesic_amd.svi import GLMReparamSVI
    B, D, seed, lr, tau = 1029, 256, 1234, 0.01, 2.0
    batches = [_regression_data(link, B, D, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, y0, o0, v0 = dev[0]
    model = GLMReparamSVI(X0, y0, link=link, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=tau,
                          ctx=ctx, offset=o0, weights=v0)
    lam = glm.init_lam(D)
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
            lam, m1, m2, elbo, grad = ref.step(link, lam, m1, m2, t, batches[k][0], batches[k][1], S, seed, 10.0 * B,
                                               lr, tau, offset=batches[k][2], weights=batches[k][3])
            if t in (1, 2, 3, 10, 20):
                ctx.sync()
                g = model.grad.cpu().numpy()
                npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
                assert np.abs(g - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert ("bsc_glm_pass_update_obs" in calls) == (S == 8) and ("bsc_glm_data_pass_obs" in calls) == (S == 11)
    assert "bsc_glm_pass_update" not in calls and "bsc_glm_data_pass" not in calls


@pytest.mark.parametrize("link", LINKS)
def test_five_updates_of_the_full_guide(ctx, link):
    from bayesic_amd.svi import GLMReparamSVI
    B, D, S, seed, lr, n_total, tau = 1029, 64, 8, 21, 0.02, 20000.0, 1.5
    X, y, o, v = _regression_data(link, B, D, 5)
    model = GLMReparamSVI(X, y, link=link, n_total=n_total, n_samples=S, seed=seed, lr=lr, prior_precision=tau, ctx=ctx,
                          covariance="full", offset=o, weights=v)
    lam = full_ref.init_lam(D)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 6):
        assert model.step() is None
        eps = full_ref.noise(D, S, seed, t - 1)
        W = full_ref.draw(lam, eps)
        ell, G = ref.data_pass(link, X, y, W, o, v)
        lam, m1, m2, elbo, _ = full_ref.finish(lam, m1, m2, t, eps, W, ell, G, n_total / B, tau, lr)
        ctx.sync()
        npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
        npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=1e-4)


def test_set_batch_with_and_without_the_vectors(ctx):
    """A batch without them goes back to the shipped entry points; raw pointers are taken as they are."""
    from bayesic_amd.svi import GLMReparamSVI
    link, B, D, S = "logistic", 325, 64, 8
    X, y, o, v = _regression_data(link, B, D, 7)
    Xd, yd, od, vd = (ctx.to_device(a) for a in (X, y, o, v))
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        plain = GLMReparamSVI(Xd, yd, link=link, n_samples=S, seed=3, ctx=ctx)
        plain.step()
        plain.set_batch(Xd, yd)
        plain.step()
        assert not plain.has_offset and not [c for c in calls if c.endswith("_obs")]
        a = GLMReparamSVI(Xd, yd, link=link, n_samples=S, seed=3, ctx=ctx, offset=od, weights=vd)
        b = GLMReparamSVI(Xd, yd, link=link, n_samples=S, seed=3, ctx=ctx)
        b.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, offset=od.data_ptr(), weights=vd.data_ptr())
        for m in (a, b):
            m.step()
            m.data_pass()
        ctx.sync()
        npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
        npt.assert_array_equal(a.stats.cpu().numpy(), b.stats.cpu().numpy())
        n_obs = len([c for c in calls if c.endswith("_obs")])
        assert n_obs == 4
        a.set_batch(Xd, yd)                      # the vectors are dropped with the batch that carried them
        a.step()
        assert calls[-1] == "bsc_glm_pass_update" and a.offset is None and a.weights is None
    finally:
        ctx.call = real_call
    with pytest.raises(ValueError, match="finite and >= 0"):
        a.set_batch(Xd, yd, weights=-vd - 1.0)
    bad = vd.clone()
    bad[5] = float("nan")
    with pytest.raises(ValueError, match="finite and >= 0"):
        a.set_batch(Xd, yd, weights=bad)
    with pytest.raises(ValueError, match="finite and >= 0"):
        GLMReparamSVI(Xd, yd, link=link, ctx=ctx, weights=bad)
    with pytest.raises(ValueError, match=r"offset must be \[325\]"):
        a.set_batch(Xd, yd, offset=od[:-1])
