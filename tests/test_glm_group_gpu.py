"""GPU parity of the random-intercept GLM route (csrc/bsc_glm_group.hip through the C ABI, svi/hier_glm.py) against
the float64 restatement in tests/_glm_group_ref.py.

Tolerances are tests/test_glm_obs_gpu.py's, with the intercept in the logit:
 * ell: |dev - ref| <= 2e-5 * sum_n v_n (|y_n l_ns| + A(l_ns) + 1), rows of weight 0 left out;
 * G: rtol 1e-4, atol 1e-4 * max|G|;
 * H: the bound of a column of G, the column being group j's indicator (H is that column of the one-hot design):
   rtol 1e-4, atol 1e-4 * max|H|;
 * extreme logits: rtol 1e-6; one row's ell against its closed form: 1e-6 (|y l| + A + 1), sixteen float32 roundings;
 * the finish from given statistics (float64 both sides): rtol 1e-9 (tests/test_glm_gpu.py's);
 * twenty updates against the reference: ELBO rtol 1e-6, gradient 1e-4 * max|grad|, lam atol 2e-4 (the same file's).
Exact accounting is compared with ==: with W = 0 and Bz = 0 every logistic residual is +-1/2, so H is a sum of halves.
Poisson inputs keep |l| <= 4, except where a test is about a wild link value.

Shapes are the smallest that reach each path: B in {1, 15, 16, 17, 37, 1003} (around one 16-row tile, several blocks),
D in {8, 64, 252, 256}, J in {1, 3, 1000} (more groups than rows among them), S in {1, 8, 11} (11 = two launches);
batches sized from the device's CU count for 2 and 3 tiles per wave; one group longer than three plan segments."""
import ctypes
import math
import re

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_group_ref as ref
import _glm_obs_ref as obs

pytestmark = pytest.mark.gpu

LINKS = ("logistic", "poisson")
CODE = {"logistic": 0, "poisson": 1}
SENTINEL = 1.0e30      # behind the end of y / o / v: a read past B would wreck the sums


def _seg_rows():
    from bayesic_amd import _ffi
    header = open(_ffi.os.path.join(_ffi.os.path.dirname(_ffi._HERE), "include", "bayesic_hip.h")).read()
    return int(re.search(r"#define BSC_GLM_GROUP_SEG_ROWS (\d+)", header).group(1))


def _dev_vec(ctx, a, shift=False, guard=16, dtype=np.float32, sentinel=SENTINEL):
    """A host vector on the device with sentinels behind its end; ``shift``: four bytes into its buffer."""
    if a is None:
        return None
    buf = np.concatenate([[sentinel] if shift else [], a, np.full(guard, sentinel)]).astype(dtype)
    t = ctx.to_device(buf)
    return t[1:] if shift else t


def _plan(ctx, gd, B, J):
    n = ctx.lib.bsc_glm_group_plan_size(B, J)
    assert n > 0
    plan = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    n_seg = ctypes.c_int32(-1)
    ctx.call("bsc_glm_group_plan", gd, B, J, plan, ctypes.byref(n_seg))
    return plan, n_seg.value


def _pass(ctx, link, X, y, g, J, W, Bm, o=None, v=None, shift_g=False, info=None):
    """X may be a device tensor (large batches are made on the device); everything else host arrays."""
    B, D = X.shape
    S = W.shape[0]
    Xd = X if isinstance(X, torch.Tensor) else ctx.to_device(X)
    Wd, Bz = ctx.to_device(W), ctx.to_device(ref.chunked(Bm))
    yd, od, vd = (_dev_vec(ctx, a) for a in (y, o, v))
    gd = _dev_vec(ctx, g, shift_g, dtype=np.int32, sentinel=-1)       # an id read past B would gather nothing
    plan, n_seg = _plan(ctx, gd, B, J)
    if info is not None:
        info["n_segments"] = n_seg
    f64 = torch.float64
    ell, G = torch.full((S,), 7.0, dtype=f64, device=ctx.device), torch.full((S, D), 7.0, dtype=f64, device=ctx.device)
    H = torch.full((S, J), 7.0, dtype=f64, device=ctx.device)
    ctx.call("bsc_glm_data_pass_groups", CODE[link], Xd, Xd.stride(0), yd, od, vd, gd, plan, B, D, J, Wd, Bz, S, ell, G, H)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), H.cpu().numpy()


def _inputs(link, B, D, J, S, seed, mode="both"):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    Bm = (0.5 * rs.standard_normal((S, J))).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if B > 1:
        v[1] = 0.5
    if link == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, g, W, Bm, o)).max() if B else 0.0
        if peak > 3.5:
            W, Bm, o = ((a * (3.5 / peak)).astype(np.float32) for a in (W, Bm, o))
    return X, y, g, W, Bm, (o if mode != "none" else None), (v if mode != "none" else None)


def _assert_close(link, got, X, y, g, J, W, Bm, o, v, what=""):
    ell, G, H = got
    ell_r, G_r, H_r = ref.data_pass(link, X, y, g, J, W, Bm, o, v)
    bound = ref.ell_bound(link, X, y, g, W, Bm, o, v)
    err = np.abs(ell - ell_r)
    print("%s %s B=%d D=%d J=%d S=%d: ell err/bound %.3g, G err/max %.3g, H err/max %.3g" % (
        what, link, X.shape[0], X.shape[1], J, W.shape[0], (err / (bound + 1e-300)).max(),
        np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300), np.abs(H - H_r).max() / (np.abs(H_r).max() + 1e-300)))
    assert (err <= 2e-5 * bound + 1e-12).all(), (err / (bound + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    npt.assert_allclose(H, H_r, rtol=1e-4, atol=1e-4 * np.abs(H_r).max())
    counts = np.bincount(g, minlength=J)
    assert (H[:, counts == 0] == 0.0).all()             # a group without rows gets exactly 0


def _check(ctx, link, X, y, g, J, W, Bm, o, v, **kw):
    if link == "poisson":
        assert np.abs(ref.logits(X, g, W, Bm, o)).max() <= 4.0
    got = _pass(ctx, link, X, y, g, J, W, Bm, o, v, **kw)
    _assert_close(link, got, X, y, g, J, W, Bm, o, v)
    return got


# ---- parity over the envelope ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["both", "none"])
@pytest.mark.parametrize("S", [1, 8, 11])
@pytest.mark.parametrize("D", [8, 64, 252, 256])
@pytest.mark.parametrize("link", LINKS)
def test_pass_matches_the_reference(ctx, link, D, S, mode):
    """Every (B, J) of the envelope's corners at this (link, D, S), with and without offset and weights."""
    for B in (1, 15, 16, 17, 37, 1003):
        for J in (1, 3, 1000):
            X, y, g, W, Bm, o, v = _inputs(link, B, D, J, S, seed=B * 7 + D + S + J, mode=mode)
            _check(ctx, link, X, y, g, J, W, Bm, o, v)


@pytest.mark.parametrize("link", LINKS)
def test_against_the_shipped_kernel_on_the_one_hot_design(ctx, link):
    """D = 8, J = 8: [X | onehot(g)] at D' = 16 through bsc_glm_data_pass_obs gives ell, G in its first eight columns
    and H^T in its last eight; the grouped pass agrees with it, each within its bound of the same reference."""
    B, D, J, S = 1003, 8, 8, 8
    X, y, g, W, Bm, o, v = _inputs(link, B, D, J, S, seed=21)
    ell, G, H = _check(ctx, link, X, y, g, J, W, Bm, o, v)
    X2 = np.concatenate([X, ref.onehot(g, J)], axis=1)
    W2 = np.concatenate([W, Bm], axis=1)
    e2, G2 = ctx.zeros(S, torch.float64), ctx.zeros((S, D + J), torch.float64)
    ctx.call("bsc_glm_data_pass_obs", CODE[link], ctx.to_device(X2), D + J, _dev_vec(ctx, y), _dev_vec(ctx, o),
             _dev_vec(ctx, v), B, D + J, ctx.to_device(W2), S, e2, G2)
    ctx.sync()
    e2, G2 = e2.cpu().numpy(), G2.cpu().numpy()
    _assert_close(link, (e2, G2[:, :D], G2[:, D:]), X, y, g, J, W, Bm, o, v, what="shipped kernel, one-hot design")
    bound = ref.ell_bound(link, X, y, g, W, Bm, o, v)
    assert (np.abs(ell - e2) <= 2 * 2e-5 * bound).all()
    H_r = ref.data_pass(link, X, y, g, J, W, Bm, o, v)[2]
    npt.assert_allclose(H, G2[:, D:], rtol=2e-4, atol=2e-4 * np.abs(H_r).max())


# ---- exact accounting -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


def _exact(ctx, B, D, g, J, seed, info=None):
    """W = 0, Bz = 0, logistic, y in {0, 1}: every residual is +-1/2 and H[s, j] = sum_{n in j} (y_n - 1/2) exactly."""
    S = 8
    rs = np.random.RandomState(seed)
    y = (rs.uniform(size=B) < 0.4).astype(np.float32)
    X = torch.rand((B, D), dtype=torch.float32, device=ctx.device)      # W = 0: the logits are 0 whatever X holds
    W, Bm = np.zeros((S, D), np.float32), np.zeros((S, J), np.float32)
    ell, _, H = _pass(ctx, "logistic", X, y, g, J, W, Bm, info=info)
    want = np.zeros(J)
    np.add.at(want, g, y.astype(np.float64) - 0.5)
    for s in range(S):
        npt.assert_array_equal(H[s], want)
    npt.assert_allclose(ell, -B * math.log(2.0), rtol=1e-6)
    return H


@pytest.mark.parametrize("D", [256, 64])
def test_group_sums_are_exact_with_empty_groups(ctx, D):
    B, J = 1003, 37
    rs = np.random.RandomState(D)
    g = rs.choice(np.arange(0, J, 3), size=B).astype(np.int32)            # two groups in three have no rows
    H = _exact(ctx, B, D, g, J, seed=D)
    empty = np.bincount(g, minlength=J) == 0
    assert empty.sum() == 24 and (H[:, empty] == 0.0).all() and (np.abs(H[:, ~empty]).sum() > 0)


@pytest.mark.parametrize("kernel,D,n_iter", [("mfma", 256, 2), ("mfma", 256, 3), ("valu", 64, 2), ("valu", 64, 3)])
def test_group_sums_are_exact_with_several_tiles_per_wave(ctx, cu, kernel, D, n_iter):
    """B = (n_iter - 1) sweeps of the resident waves + one tile + 5 rows (tests/test_regression_multi_tile_gpu.py's
    form): the tail tiles of the last iteration run past the batch and their residual stores must not land."""
    rows = 16 if kernel == "mfma" else 8
    B = (n_iter - 1) * 8 * cu * rows + rows + 5
    n_tiles = (B + rows - 1) // rows
    assert (n_tiles + 8 * cu - 1) // (8 * cu) == n_iter
    J = 1000
    g = np.random.RandomState(n_iter).randint(J, size=B).astype(np.int32)
    _exact(ctx, B, D, g, J, seed=n_iter + D)


@pytest.mark.parametrize("D", [256, 64])
def test_a_group_longer_than_three_segments_is_summed_in_segment_order(ctx, D):
    cap = _seg_rows()
    B, J = 3 * cap + 300, 5
    rs = np.random.RandomState(9)
    g = np.where(rs.uniform(size=B) < 0.05, rs.randint(J, size=B), 2).astype(np.int32)     # group 2 holds ~95 %
    assert (g == 2).sum() > 3 * cap
    info = {}
    _exact(ctx, B, D, g, J, seed=D + 1, info=info)
    assert info["n_segments"] >= 4 + (J - 1) > 1
    # and at parity with real residuals
    X, y, _, W, Bm, o, v = _inputs("logistic", B, D, J, 8, seed=4)
    _check(ctx, "logistic", X, y, g, J, W, Bm, o, v)


# ---- the forward gather ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("link", LINKS)
def test_each_row_gathers_its_own_groups_intercept(ctx, link, D):
    """W = 0, distinct Bz[j][s], all weights zero except one row: ell_s = v (y l - A(l)) at l = Bz[g_row][s].  Rows of
    the first, a middle and the last (partial) tile, S = 11 so that both chunks of Bz are read."""
    B, J, S = 1003, 13, 11
    rs = np.random.RandomState(D)
    X = rs.standard_normal((B, D)).astype(np.float32)
    g = ((np.arange(B) * 7 + 3) % J).astype(np.int32)
    y = (np.arange(B) % 2).astype(np.float32) if link == "logistic" else (np.arange(B) % 3).astype(np.float32)
    W = np.zeros((S, D), np.float32)
    Bm = (0.125 * (np.arange(S)[:, None] * J + np.arange(J)[None, :]) - 2.0).astype(np.float32) * np.float32(0.25)
    assert len(np.unique(Bm)) == S * J and np.abs(Bm).max() <= 4.0
    for row in (0, 9, 509, 997, 1002):
        v = np.zeros(B, np.float32)
        v[row] = 2.0
        ell, G, H = _pass(ctx, link, X, y, g, J, W, Bm, None, v)
        l = Bm[:, g[row]].astype(np.float64)
        A, dA = obs.glm.log_partition(link, l)
        want = 2.0 * (y[row] * l - A)
        assert (np.abs(ell - want) <= 1e-6 * 2.0 * (np.abs(y[row] * l) + A + 1.0)).all(), (row, ell, want)
        # the one residual lands in the row's group and nowhere else
        r = 2.0 * (y[row] - dA)
        npt.assert_allclose(H[:, g[row]], r, rtol=1e-5, atol=1e-6)
        others = np.ones(J, bool)
        others[g[row]] = False
        assert (H[:, others] == 0.0).all()
        npt.assert_allclose(G, r[:, None] * X[row].astype(np.float64)[None, :], rtol=1e-5, atol=1e-5)


# ---- other pass checks ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("link", LINKS)
def test_misaligned_group_ids_take_the_eight_row_kernel(ctx, link):
    """D = 256: g four bytes into its buffer takes the 8-row kernel (the MFMA kernel loads ids sixteen bytes at a
    time); both agree with the reference, which they would not if misaligned ids were read sixteen bytes at a time."""
    X, y, g, W, Bm, o, v = _inputs(link, 1003, 256, 37, 8, seed=3)
    a = _check(ctx, link, X, y, g, 37, W, Bm, o, v)
    b = _check(ctx, link, X, y, g, 37, W, Bm, o, v, shift_g=True)
    bound = ref.ell_bound(link, X, y, g, W, Bm, o, v)
    assert (np.abs(a[0] - b[0]) <= 2 * 2e-5 * bound).all()


@pytest.mark.parametrize("D,B", [(256, 200), (64, 64)])
def test_logistic_at_extreme_logits_through_the_intercept(ctx, D, B):
    """Logits of +-80 that come from the intercept alone (W = 0)."""
    S, J = 8, 6
    X = np.random.RandomState(D).standard_normal((B, D)).astype(np.float32)
    W = np.zeros((S, D), np.float32)
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(J)[None, :])
    Bm = (80.0 * sign).astype(np.float32)
    g = (np.arange(B) % J).astype(np.int32)
    y = ((np.arange(B) // 2) % 2).astype(np.float32)
    v = (1.0 + (np.arange(B) % 3)).astype(np.float32)
    ell, G, H = _pass(ctx, "logistic", X, y, g, J, W, Bm, None, v)
    assert np.isfinite(ell).all() and np.isfinite(G).all() and np.isfinite(H).all()
    ell_r, G_r, H_r = ref.data_pass("logistic", X, y, g, J, W, Bm, None, v)
    npt.assert_allclose(ell, ell_r, rtol=1e-6)
    npt.assert_allclose(H, H_r, rtol=1e-6, atol=1e-30)
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())     # sums of signed x: the parity bound


@pytest.mark.parametrize("D", [256, 64])
def test_zero_weight_rows_at_a_wild_poisson_logit_are_neutral(ctx, D):
    """The rows of one group have weight 0 and a logit of 200 through that group's intercept (exp overflows float32):
    ell, G and H stay finite, equal the pass without those rows, and the group's H is exactly 0."""
    link, B, J = "poisson", 165, 7
    X, y, g, W, Bm, o, v = _inputs(link, B, D, J, 8, seed=D)
    wild = g == 4
    assert 5 < wild.sum() < B
    v[wild] = 0.0
    Bm[:, 4] = 200.0
    got = _pass(ctx, link, X, y, g, J, W, Bm, o, v)
    assert all(np.isfinite(a).all() for a in got)
    assert (got[2][:, 4] == 0.0).all()
    keep = ~wild
    ell_r, G_r, H_r = ref.data_pass(link, X[keep], y[keep], g[keep], J, W, Bm, o[keep], v[keep])
    bound = ref.ell_bound(link, X[keep], y[keep], g[keep], W, Bm, o[keep], v[keep])
    assert (np.abs(got[0] - ell_r) <= 2e-5 * bound).all()
    npt.assert_allclose(got[1], G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    npt.assert_allclose(got[2], H_r, rtol=1e-4, atol=1e-4 * np.abs(H_r).max())


@pytest.mark.parametrize("B,D,S", [(325, 256, 11), (165, 64, 8)])
@pytest.mark.parametrize("link", LINKS)
def test_with_zero_intercepts_ell_and_G_are_the_obs_pass_bit_for_bit(ctx, link, B, D, S):
    J = 9
    X, y, g, W, _, o, v = _inputs(link, B, D, J, S, seed=9)
    got = _pass(ctx, link, X, y, g, J, W, np.zeros((S, J), np.float32), o, v)
    ell, G = ctx.zeros(S, torch.float64), ctx.zeros((S, D), torch.float64)
    ctx.call("bsc_glm_data_pass_obs", CODE[link], ctx.to_device(X), D, _dev_vec(ctx, y), _dev_vec(ctx, o),
             _dev_vec(ctx, v), B, D, ctx.to_device(W), S, ell, G)
    ctx.sync()
    npt.assert_array_equal(got[0], ell.cpu().numpy())
    npt.assert_array_equal(got[1], G.cpu().numpy())


@pytest.mark.parametrize("link", LINKS)
def test_two_runs_are_bit_identical(ctx, link):
    X, y, g, W, Bm, o, v = _inputs(link, 1029, 256, 37, 11, seed=5)
    a = _pass(ctx, link, X, y, g, 37, W, Bm, o, v)
    b = _pass(ctx, link, X, y, g, 37, W, Bm, o, v)
    for p, q in zip(a, b):
        npt.assert_array_equal(p, q)


def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9), ctx.zeros((65, 260))
    o, v, Bz = ctx.zeros(12), ctx.zeros(12), ctx.zeros(9 * 8 * 8)
    g = torch.zeros(12, dtype=torch.int32, device=ctx.device)
    plan, _ = _plan(ctx, g, 8, 3)
    ell, G, H = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros((65, 8), f64)

    def call(link=0, Xa=X, ldx=256, D=256, S=8, J=3, plan_=plan, Ha=H, ya=y):
        ctx.call("bsc_glm_data_pass_groups", link, Xa, ldx, ya, o, v, g, plan_, 8, D, J, W, Bz, S, ell, G, Ha)

    who = "bsc_glm_data_pass_groups"
    with pytest.raises(BayesicHipError, match=who + ": J=0 must be in"):
        call(J=0)
    with pytest.raises(BayesicHipError, match=who + ": J=65537 must be in"):
        call(J=65537)
    with pytest.raises(BayesicHipError, match=who + ": plan is null"):
        call(plan_=None)
    with pytest.raises(BayesicHipError, match=who + ": H is null"):
        call(Ha=None)
    # the inherited envelope
    with pytest.raises(BayesicHipError, match=who + ": y is null with B=8"):
        call(ya=None)
    with pytest.raises(BayesicHipError, match=who + ": D=6 must be a multiple of 4"):
        call(ldx=8, D=6)
    with pytest.raises(BayesicHipError, match="D=260 must be a multiple of 4 in"):
        call(ldx=260, D=260)
    with pytest.raises(BayesicHipError, match="16-byte aligned"):
        call(Xa=X.view(-1)[1:])
    with pytest.raises(BayesicHipError, match="S=65"):
        call(link=1, S=65)
    with pytest.raises(BayesicHipError, match="link=2"):
        call(link=2)
    with pytest.raises(BayesicHipError, match="ldx=6"):
        call(ldx=6, D=8)
    # the plan: ids outside [0, J) are refused with the first offending row
    bad = torch.tensor([0, 1, 2, 3, 1, 0], dtype=torch.int32, device=ctx.device)
    with pytest.raises(BayesicHipError, match=r"row 3 has group id 3 outside \[0,3\)"):
        _plan(ctx, bad, 6, 3)
    with pytest.raises(BayesicHipError, match="bsc_glm_hier_update: stats is null"):
        ctx.call("bsc_glm_hier_update", None, ell, G, ell, G, ell, W, Bz, 8, 3, 8, 1.0, 1.0, 1.0, 1.0, 1, 0.01, 0.9,
                 0.999, 1e-8, 1, 1, None, 1, None, None, ell, G)
    ctx.sync()


# ---- the finish -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ready", [1, 0])
@pytest.mark.parametrize("S", [8, 11])
@pytest.mark.parametrize("J", [1, 1000])
def test_finish_from_given_statistics(ctx, J, S, ready):
    """bsc_glm_hier_update(stats): float64 on both sides."""
    D = 24
    P = D + J + 1
    rs = np.random.RandomState(J + S)
    f64 = torch.float64
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    m1, m2 = 0.01 * rs.standard_normal(2 * P), 1e-4 * rs.uniform(size=2 * P)
    ell, G, H = -100.0 * rs.uniform(1, 2, S), rs.standard_normal((S, D)) * 5, rs.standard_normal((S, J)) * 3
    seed, t, scale, tau, a0, b0, lr = 99, 4, 12.5, 0.7, 1.5, 0.8, 0.02
    eps, eps_n = ref.noise(D, J, S, seed, t - 1), ref.noise(D, J, S, seed, t)
    W, Bm, zeta = ref.draw(lam, eps, D, J)
    n_bz = ((S + 7) // 8) * J * 8
    d = dict(stats=ctx.to_device(np.concatenate([ell, G.ravel(), H.ravel()]), f64), lam=ctx.to_device(lam, f64),
             out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64), m2=ctx.to_device(m2, f64),
             eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()), Bz=ctx.to_device(ref.chunked(Bm)),
             eps_n=ctx.to_device(eps_n.ravel() if ready else np.zeros(S * P), f64), W_n=ctx.zeros(S * D),
             Bz_n=torch.full((n_bz,), 5.0, dtype=torch.float32, device=ctx.device), elbo=ctx.zeros(1, f64),
             grad=ctx.zeros(2 * P, f64))
    ctx.call("bsc_glm_hier_update", d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["Bz"], D, J, S,
             scale, tau, a0, b0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], ready, d["W_n"], d["Bz_n"], d["elbo"],
             d["grad"])
    ctx.sync()
    lam_r, m1_r, m2_r, elbo_r, grad_r = ref.finish(lam, m1, m2, t, eps, W, Bm, zeta, ell, G, H, scale, tau, a0, b0, lr)
    npt.assert_allclose(d["elbo"].item(), elbo_r, rtol=1e-9)
    npt.assert_allclose(d["grad"].cpu().numpy(), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
    npt.assert_allclose(d["out"].cpu().numpy(), lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(d["m1"].cpu().numpy(), m1_r, rtol=1e-9, atol=1e-15)
    npt.assert_allclose(d["m2"].cpu().numpy(), m2_r, rtol=1e-9, atol=1e-18)
    npt.assert_allclose(d["lam"].cpu().numpy(), lam, rtol=0, atol=0)       # lam_in is not modified
    npt.assert_allclose(d["eps_n"].cpu().numpy().reshape(S, P), eps_n, rtol=1e-12, atol=1e-14)
    # the next draws: float32-rounded from float64 on both sides (1 ulp where the float64 values straddle a tie)
    W_r, Bm_r, _ = ref.draw(lam_r, eps_n, D, J)
    npt.assert_allclose(d["W_n"].cpu().numpy().reshape(S, D), W_r, rtol=2e-7, atol=1e-9)
    Bz_n = d["Bz_n"].cpu().numpy()
    npt.assert_allclose(ref.unchunk(Bz_n, S, J), Bm_r, rtol=2e-7, atol=1e-9)
    assert (Bz_n.reshape(-1, J, 8)[-1][:, S - 8 * ((S - 1) // 8):] == 0.0).all()      # the unused slots are zeroed


# ---- the driver -----------------------------------------------------------------------------------------------------

def _hierarchy(link, B, D, J, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    o = (0.5 * rs.standard_normal(B)).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    L = X.astype(np.float64) @ rs.standard_normal(D) + 0.7 * rs.standard_normal(J)[g] + o
    if link == "logistic":
        y = (rs.uniform(size=B) < 1.0 / (1.0 + np.exp(-L))).astype(np.float32)
    else:
        y = rs.poisson(np.exp(np.minimum(L, 3.0))).astype(np.float32)
    return X, y, g, o, v


@pytest.mark.parametrize("S", [8, 11])
@pytest.mark.parametrize("link", LINKS)
def test_twenty_updates_track_the_reference_over_two_batches(ctx, link, S):
    """set_batch with new rows, new groups, new offsets and weights before every update."""
    from bayesic_amd.svi import HierGLMReparamSVI
    B, D, J, seed, lr, tau, a0, b0 = 1029, 256, 20, 1234, 0.01, 2.0, 1.5, 0.8
    batches = [_hierarchy(link, B, D, J, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    X0, y0, g0, o0, v0 = dev[0]
    model = HierGLMReparamSVI(X0, y0, g0, J, link=link, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr,
                              prior_precision=tau, a0=a0, b0=b0, offset=o0, weights=v0, ctx=ctx)
    P = D + J + 1
    lam = ref.init_lam(P)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    for t in range(1, 21):
        k = (t - 1) % 2
        Xk, yk, gk, ok, vk = dev[k]
        model.set_batch(Xk, yk, offset=ok, weights=vk, groups=gk)
        assert model.step() is None
        Xh, yh, gh, oh, vh = batches[k]
        lam, m1, m2, elbo, grad = ref.step(link, lam, m1, m2, t, Xh, yh, gh, J, S, seed, 10.0 * B, lr, tau, a0, b0,
                                           offset=oh, weights=vh)
        if t in (1, 2, 3, 10, 20):
            ctx.sync()
            gd = model.grad.cpu().numpy()
            npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
            assert np.abs(gd - grad).max() <= 1e-4 * np.abs(grad).max()
            npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    p = model.params()
    npt.assert_allclose(np.concatenate([p["m"], p["rho"]]), lam, atol=2e-4)
    assert p["w"][0].shape == (D,) and p["b"][1].shape == (J,) and np.isscalar(p["zeta"][0].item())
    npt.assert_array_equal(p["b"][0], p["m"][D:D + J])


def test_set_batch_and_refusals_of_the_driver(ctx):
    from bayesic_amd._ffi import BayesicHipError
    from bayesic_amd.svi import HierGLMReparamSVI
    B, D, J = 325, 64, 5
    X, y, g, o, v = _hierarchy("logistic", B, D, J, 7)
    Xd, yd, gd = ctx.to_device(X), ctx.to_device(y), ctx.to_device(g)
    a = HierGLMReparamSVI(Xd, yd, gd, J, n_samples=8, seed=3, ctx=ctx)
    b = HierGLMReparamSVI(Xd, yd, g, J, n_samples=8, seed=3, ctx=ctx)                 # host ids are uploaded
    b.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, groups=gd.data_ptr())          # raw pointers are taken as they are
    for m in (a, b):
        m.step()
        m.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    assert a.n_segments == len(np.unique(g))
    # new groups: the plan is rebuilt and the next update sees them
    g2 = ((g + 1) % J).astype(np.int32)
    a.set_batch(Xd, yd, groups=ctx.to_device(g2))
    a.data_pass()
    ctx.sync()
    W = a.W.cpu().numpy().reshape(8, D)
    Bm = ref.unchunk(a.Bz.cpu().numpy(), 8, J)
    H_r = ref.data_pass("logistic", X, y, g2, J, W, Bm)[2]
    npt.assert_allclose(a.H.cpu().numpy().reshape(8, J), H_r, rtol=1e-4, atol=1e-4 * np.abs(H_r).max())
    with pytest.raises(ValueError, match="set_batch needs groups="):
        a.set_batch(Xd, yd)
    bad = g.copy()
    bad[17] = J
    with pytest.raises(BayesicHipError, match=r"row 17 has group id 5 outside \[0,5\)"):
        a.set_batch(Xd, yd, groups=ctx.to_device(bad))
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        a.predict(Xd)
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        a.heldout_lpd(Xd, yd)
    with pytest.raises(ValueError, match="mean-field guide only"):
        HierGLMReparamSVI(Xd, yd, gd, J, covariance="full", ctx=ctx)
