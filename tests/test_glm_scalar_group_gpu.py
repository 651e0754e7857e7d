"""GPU parity of the random-intercept routes of the families with a learned scalar (csrc/bsc_glm_scalar_group.hip
through the C ABI, svi/hier_scalar.py) against the float64 restatement in tests/_glm_scalar_group_ref.py, which feeds
the one-hot design to the family's own helper.

Tolerances are the families' and tests/test_glm_group_gpu.py's, not new ones:
 * ell and T: |dev - ref| <= 2e-5 * the family reference's bounds on the one-hot design;
 * G and H: rtol 1e-4, atol 1e-4 * max;
 * the finish from given statistics (float64 both sides): rtol 1e-9;
 * twenty updates against the reference: gradient 1e-4 * max|grad|, lam atol 2e-4, and the ELBO by each family's own
   criterion -- negbin: rtol 1e-6 of the ELBO itself on low-mean counts, with the condition number size / |ELBO| <= 4
   asserted from the reference (tests/test_glm_nb_gpu.py's); gamma and weibull: within 1e-6 of scale * mean_s b_ell[s],
   the size of the data terms (their tests' criterion without the sizes of the prior's terms, so no looser than theirs).
Compared with ==: Bz = 0 against the family's ungrouped pass, empty groups, two runs, and the exact accounting of the
Weibull link at W = 0, Bz = 0, tau = 0, y = +-1 with small integer weights and X (z = 0, e^z = 1, r = v (1 - delta):
H[s,j] = the censored weight of group j, T[s] = the event weight, ell[s] = -sum v, G = r^T X).

Shapes are the smallest that reach each path (tests/test_glm_group_gpu.py's): B in {1, 15, 16, 17, 37, 1003}, D in
{8, 64, 252, 256}, J in {1, 3, 1000}, S in {1, 8, 11} (11 = two launches with a partly filled chunk: tau, Bz and T of
the second chunk must pair up); batches sized from the device's CU count for 2 and 3 tiles per wave in both tile
shapes; one group longer than three plan segments; sentinels behind y, o, v, g and logtau; tau inside each family's
accuracy envelope."""
import ctypes
import math
import re

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_scalar_group_ref as ref

pytestmark = pytest.mark.gpu

FAMILIES = ref.FAMILIES
CODE = ref.CODE
UNGROUPED = {"negbin": "bsc_glm_nb_data_pass", "gamma": "bsc_glm_gamma_data_pass",
             "weibull": "bsc_glm_weibull_data_pass"}
SENTINEL = 1.0e30      # behind the end of y / o / v / logtau: a read past the end would wreck the sums


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
    return t[1:1 + len(a) + guard] if shift else t


def _plan(ctx, gd, B, J):
    n = ctx.lib.bsc_glm_group_plan_size(B, J)
    assert n > 0
    plan = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    n_seg = ctypes.c_int32(-1)
    ctx.call("bsc_glm_group_plan", gd, B, J, plan, ctypes.byref(n_seg))
    return plan, n_seg.value


def _pass(ctx, fam, X, y, g, J, W, Bm, logtau, o=None, v=None, shift_g=False, info=None):
    """X may be a device tensor (large batches are made on the device); everything else host arrays."""
    B, D = X.shape
    S = W.shape[0]
    Xd = X if isinstance(X, torch.Tensor) else ctx.to_device(X)
    Wd, Bz = ctx.to_device(W), ctx.to_device(ref.chunked(Bm))
    yd, od, vd, td = (_dev_vec(ctx, a) for a in (y, o, v, logtau))
    gd = _dev_vec(ctx, g, shift_g, dtype=np.int32, sentinel=-1)       # an id read past B would gather nothing
    plan, n_seg = _plan(ctx, gd, B, J)
    if info is not None:
        info["n_segments"] = n_seg
    f64 = torch.float64
    ell, G = torch.full((S,), 7.0, dtype=f64, device=ctx.device), torch.full((S, D), 7.0, dtype=f64, device=ctx.device)
    H, T = torch.full((S, J), 7.0, dtype=f64, device=ctx.device), torch.full((S,), 7.0, dtype=f64, device=ctx.device)
    ctx.call("bsc_glm_scalar_data_pass_groups", CODE[fam], Xd, Xd.stride(0), yd, od, vd, gd, plan, B, D, J, Wd, Bz, td,
             S, ell, G, H, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), H.cpu().numpy(), T.cpu().numpy()


def _ungrouped(ctx, fam, X, y, W, logtau, o, v):
    B, D = X.shape
    S = W.shape[0]
    f64 = torch.float64
    ell, G, T = ctx.zeros(S, f64), ctx.zeros((S, D), f64), ctx.zeros(S, f64)
    ctx.call(UNGROUPED[fam], ctx.to_device(X), D, _dev_vec(ctx, y), _dev_vec(ctx, o), _dev_vec(ctx, v), B, D,
             ctx.to_device(W), _dev_vec(ctx, logtau), S, ell, G, T)
    ctx.sync()
    return ell.cpu().numpy(), G.cpu().numpy(), T.cpu().numpy()


def _inputs(fam, B, D, J, S, seed, mode="both"):
    """The families' own recipes (tests/_glm_nb_ref.make_inputs and its two siblings) with the intercept in the logit:
    X ~ N / sqrt(D), W ~ 0.6 N, Bm ~ 0.5 N, offsets N(0, 1), weights U(0, 3) with every fifth exactly zero, tau spread
    over the family's accuracy envelope; negbin: NB(2, mean 1.5) counts, every seventh from [100, 3000); gamma:
    Gamma(2, mean e^l) at the first draw's logit, every seventh times 1000 and every eleventh times 1e-3; weibull:
    Weibull(1.5, e^l), three in ten censored, all durations scaled so that z <= 60 on every kept (row, draw), and the
    rows of weight 0 hold y = 0 and NaN in turn.  Returns (X, y, g, W, Bm, logtau, o, v)."""
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
    use = mode != "none"
    lo, hi = ref.TAU_RANGE[fam]
    logtau = (np.linspace(lo, hi, S)[rs.permutation(S)] if S > 1 else np.array([0.5])).astype(np.float32)
    L = ref.grp.logits(X, g, W, Bm, o if use else None)
    if fam == "negbin":
        y = rs.negative_binomial(2, 2.0 / 3.5, size=B).astype(np.float64)
        big = rs.randint(100, 3000, size=B)
        y[6::7] = big[6::7]
    elif fam == "gamma":
        y = rs.gamma(2.0, np.exp(L[:, 0]) / 2.0)
        y[6::7] *= 1000.0
        y[3::11] *= 1.0e-3
        y = np.maximum(y, 1.0e-30)
    else:
        t = np.exp(L[:, 0]) * rs.weibull(1.5, B)
        cens = rs.uniform(size=B) < 0.3
        t = np.maximum(np.where(cens, t * rs.uniform(0.1, 1.0, B), t), 1.0e-30)
        k = np.exp(logtau.astype(np.float64))[None, :]
        keep = (v > 0) if use else np.ones(B, bool)
        over = (np.log(t)[:, None] - L - 60.0 / k)[keep].max() if keep.any() else 0.0
        t = t * math.exp(-max(over, 0.0) - 1e-3)
        y = np.where(cens, -t, t)
        if use:
            dead = np.flatnonzero(v == 0)
            y[dead[0::2]] = 0.0
            y[dead[1::2]] = np.nan
    return X, y.astype(np.float32), g, W, Bm, logtau, (o if use else None), (v if use else None)


def _assert_close(fam, got, X, y, g, J, W, Bm, logtau, o, v, what=""):
    ell, G, H, T = got
    ell_r, G_r, H_r, T_r = ref.data_pass(fam, X, y, g, J, W, Bm, logtau, o, v)
    b_ell, b_T = ref.bounds(fam, X, y, g, J, W, Bm, logtau, o, v)
    e_ell, e_T = np.abs(ell - ell_r), np.abs(T - T_r)
    print("%s %s B=%d D=%d J=%d S=%d: ell err/bound %.3g, T err/bound %.3g, G err/max %.3g, H err/max %.3g" % (
        what, fam, X.shape[0], X.shape[1], J, W.shape[0], (e_ell / (b_ell + 1e-300)).max(),
        (e_T / (b_T + 1e-300)).max(), np.abs(G - G_r).max() / (np.abs(G_r).max() + 1e-300),
        np.abs(H - H_r).max() / (np.abs(H_r).max() + 1e-300)))
    assert (e_ell <= 2e-5 * b_ell + 1e-12).all(), (e_ell / (b_ell + 1e-300)).max()
    assert (e_T <= 2e-5 * b_T + 1e-12).all(), (e_T / (b_T + 1e-300)).max()
    npt.assert_allclose(G, G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    npt.assert_allclose(H, H_r, rtol=1e-4, atol=1e-4 * np.abs(H_r).max())
    counts = np.bincount(g, minlength=J)
    assert (H[:, counts == 0] == 0.0).all()             # a group without rows gets exactly 0


def _check(ctx, fam, X, y, g, J, W, Bm, logtau, o, v, **kw):
    got = _pass(ctx, fam, X, y, g, J, W, Bm, logtau, o, v, **kw)
    _assert_close(fam, got, X, y, g, J, W, Bm, logtau, o, v)
    return got


# ---- parity over the envelope ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["both", "none"])
@pytest.mark.parametrize("S", [1, 8, 11])
@pytest.mark.parametrize("D", [8, 64, 252, 256])
@pytest.mark.parametrize("fam", FAMILIES)
def test_pass_matches_the_reference(ctx, fam, D, S, mode):
    """Every (B, J) of the envelope's corners at this (family, D, S), with and without offset and weights."""
    for B in (1, 15, 16, 17, 37, 1003):
        for J in (1, 3, 1000):
            args = _inputs(fam, B, D, J, S, seed=B * 7 + D + S + J, mode=mode)
            X, y, g, W, Bm, logtau, o, v = args
            _check(ctx, fam, X, y, g, J, W, Bm, logtau, o, v)


@pytest.mark.parametrize("fam", FAMILIES)
def test_against_the_shipped_kernel_on_the_one_hot_design(ctx, fam):
    """D = 8, J = 8: [X | onehot(g)] at D' = 16 through the family's ungrouped pass gives ell, T, G in its first eight
    columns and H^T in its last eight; the grouped pass agrees with it, each within its bound of the same reference."""
    B, D, J, S = 1003, 8, 8, 8
    X, y, g, W, Bm, logtau, o, v = _inputs(fam, B, D, J, S, seed=21)
    ell, G, H, T = _check(ctx, fam, X, y, g, J, W, Bm, logtau, o, v)
    e2, G2, T2 = _ungrouped(ctx, fam, ref.design(X, g, J), y, ref.draws(W, Bm), logtau, o, v)
    _assert_close(fam, (e2, G2[:, :D], G2[:, D:], T2), X, y, g, J, W, Bm, logtau, o, v,
                  what="shipped kernel, one-hot design")
    b_ell, b_T = ref.bounds(fam, X, y, g, J, W, Bm, logtau, o, v)
    assert (np.abs(ell - e2) <= 2 * 2e-5 * b_ell).all() and (np.abs(T - T2) <= 2 * 2e-5 * b_T).all()
    H_r = ref.data_pass(fam, X, y, g, J, W, Bm, logtau, o, v)[2]
    npt.assert_allclose(H, G2[:, D:], rtol=2e-4, atol=2e-4 * np.abs(H_r).max())


# ---- exact accounting -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


def _exact(ctx, B, D, g, J, seed, S=8, info=None):
    """The Weibull link at W = 0, Bz = 0, tau = 0, no offset, y = +-1, integer weights in 0 .. 3 and integer X in
    -2 .. 2: every sum is one of small integers, exact in float32 and float64."""
    rs = np.random.RandomState(seed)
    y = np.where(rs.uniform(size=B) < 0.4, -1.0, 1.0).astype(np.float32)
    v = rs.randint(0, 4, size=B).astype(np.float32)
    Xh = rs.randint(-2, 3, size=(B, D)).astype(np.float32)
    W, Bm, logtau = np.zeros((S, D), np.float32), np.zeros((S, J), np.float32), np.zeros(S, np.float32)
    ell, G, H, T = _pass(ctx, "weibull", Xh, y, g, J, W, Bm, logtau, None, v, info=info)
    v64 = v.astype(np.float64)
    r = v64 * (y < 0)
    want_H = np.zeros(J)
    np.add.at(want_H, g, r)
    for s in range(S):
        npt.assert_array_equal(H[s], want_H)
        npt.assert_array_equal(G[s], r @ Xh.astype(np.float64))
    npt.assert_array_equal(T, np.full(S, (v64 * (y > 0)).sum()))
    npt.assert_array_equal(ell, np.full(S, -v64.sum()))
    return H


@pytest.mark.parametrize("D", [256, 64])
def test_sums_are_exact_with_empty_groups(ctx, D):
    B, J = 1003, 37
    rs = np.random.RandomState(D)
    g = rs.choice(np.arange(0, J, 3), size=B).astype(np.int32)            # two groups in three have no rows
    H = _exact(ctx, B, D, g, J, seed=D, S=11)
    empty = np.bincount(g, minlength=J) == 0
    assert empty.sum() == 24 and (H[:, empty] == 0.0).all() and (np.abs(H[:, ~empty]).sum() > 0)


@pytest.mark.parametrize("kernel,D,n_iter", [("mfma", 256, 2), ("mfma", 256, 3), ("valu", 64, 2), ("valu", 64, 3)])
def test_sums_are_exact_with_several_tiles_per_wave(ctx, cu, kernel, D, n_iter):
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
    X, y, _, W, Bm, logtau, o, v = _inputs("negbin", B, D, J, 8, seed=4)
    _check(ctx, "negbin", X, y, g, J, W, Bm, logtau, o, v)


# ---- other pass checks ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
def test_misaligned_group_ids_take_the_eight_row_kernel(ctx, fam):
    """D = 256: g four bytes into its buffer takes the 8-row kernel (the MFMA kernel loads ids sixteen bytes at a
    time); both agree with the reference."""
    X, y, g, W, Bm, logtau, o, v = _inputs(fam, 1003, 256, 37, 8, seed=3)
    a = _check(ctx, fam, X, y, g, 37, W, Bm, logtau, o, v)
    b = _check(ctx, fam, X, y, g, 37, W, Bm, logtau, o, v, shift_g=True)
    b_ell = ref.bounds(fam, X, y, g, 37, W, Bm, logtau, o, v)[0]
    assert (np.abs(a[0] - b[0]) <= 2 * 2e-5 * b_ell).all()


@pytest.mark.parametrize("D", [256, 64])
@pytest.mark.parametrize("fam", FAMILIES)
def test_zero_weight_rows_at_a_wild_link_value_are_neutral(ctx, fam, D):
    """The rows of one group have weight 0 and a logit of -+200 through that group's intercept (the Gamma and Weibull
    exponentials overflow float32; the negative binomial's softplus is 200): every output stays finite and equals the
    pass without those rows within the tolerances, and the group's H is exactly 0."""
    B, J = 165, 7
    X, y, g, W, Bm, logtau, o, v = _inputs(fam, B, D, J, 8, seed=D)
    wild = g == 4
    assert 5 < wild.sum() < B
    v[wild] = 0.0
    Bm[:, 4] = 200.0 if fam == "negbin" else -200.0
    got = _pass(ctx, fam, X, y, g, J, W, Bm, logtau, o, v)
    assert all(np.isfinite(a).all() for a in got)
    assert (got[2][:, 4] == 0.0).all()
    keep = ~wild
    args = (X[keep], y[keep], g[keep], J, W, Bm, logtau, o[keep], v[keep])
    ell_r, G_r, H_r, T_r = ref.data_pass(fam, *args)
    b_ell, b_T = ref.bounds(fam, *args)
    assert (np.abs(got[0] - ell_r) <= 2e-5 * b_ell).all() and (np.abs(got[3] - T_r) <= 2e-5 * b_T).all()
    npt.assert_allclose(got[1], G_r, rtol=1e-4, atol=1e-4 * np.abs(G_r).max())
    npt.assert_allclose(got[2], H_r, rtol=1e-4, atol=1e-4 * np.abs(H_r).max())


@pytest.mark.parametrize("B,D,S", [(325, 256, 11), (165, 64, 8)])
@pytest.mark.parametrize("fam", FAMILIES)
def test_with_zero_intercepts_ell_G_and_T_are_the_ungrouped_pass_bit_for_bit(ctx, fam, B, D, S):
    """Both tile shapes: D = 256 with aligned vectors is the MFMA kernel in both passes, D = 64 the 8-row one."""
    J = 9
    X, y, g, W, _, logtau, o, v = _inputs(fam, B, D, J, S, seed=9)
    got = _pass(ctx, fam, X, y, g, J, W, np.zeros((S, J), np.float32), logtau, o, v)
    ell, G, T = _ungrouped(ctx, fam, X, y, W, logtau, o, v)
    npt.assert_array_equal(got[0], ell)
    npt.assert_array_equal(got[1], G)
    npt.assert_array_equal(got[3], T)


@pytest.mark.parametrize("fam", FAMILIES)
def test_two_runs_are_bit_identical(ctx, fam):
    X, y, g, W, Bm, logtau, o, v = _inputs(fam, 1029, 256, 37, 11, seed=5)
    a = _pass(ctx, fam, X, y, g, 37, W, Bm, logtau, o, v)
    b = _pass(ctx, fam, X, y, g, 37, W, Bm, logtau, o, v)
    for p, q in zip(a, b):
        npt.assert_array_equal(p, q)


def test_refusals_name_the_entry_point_and_the_quantity(ctx):
    from bayesic_amd._ffi import BayesicHipError
    f64 = torch.float64
    X, y, W = ctx.zeros((9, 260)), ctx.zeros(9), ctx.zeros((65, 260))
    o, v, Bz, lt = ctx.zeros(12), ctx.zeros(12), ctx.zeros(9 * 8 * 8), ctx.zeros(65)
    g = torch.zeros(12, dtype=torch.int32, device=ctx.device)
    plan, _ = _plan(ctx, g, 8, 3)
    ell, G, H = ctx.zeros(65, f64), ctx.zeros((65, 260), f64), ctx.zeros((65, 8), f64)
    T = torch.full((65,), 7.0, dtype=f64, device=ctx.device)

    def call(fam=0, Xa=X, ldx=256, D=256, S=8, J=3, plan_=plan, Ha=H, ya=y, lta=lt, Ta=T):
        ctx.call("bsc_glm_scalar_data_pass_groups", fam, Xa, ldx, ya, o, v, g, plan_, 8, D, J, W, Bz, lta, S, ell, G, Ha,
                 Ta)

    who = "bsc_glm_scalar_data_pass_groups"
    with pytest.raises(BayesicHipError, match=who + ": family=3 must be BSC_SCALAR_NEGBIN"):
        call(fam=3)
    with pytest.raises(BayesicHipError, match=who + ": J=0 must be in"):
        call(J=0)
    with pytest.raises(BayesicHipError, match=who + ": J=65537 must be in"):
        call(J=65537)
    with pytest.raises(BayesicHipError, match=who + ": plan is null"):
        call(plan_=None)
    with pytest.raises(BayesicHipError, match=who + ": H is null"):
        call(Ha=None)
    with pytest.raises(BayesicHipError, match=who + ": logtau is null"):
        call(lta=None)
    with pytest.raises(BayesicHipError, match=who + ": logtau must be 4-byte aligned"):
        call(lta=lt.data_ptr() + 2)
    with pytest.raises(BayesicHipError, match=who + ": null output"):
        call(Ta=None)
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
        call(fam=1, S=65)
    with pytest.raises(BayesicHipError, match="ldx=6"):
        call(ldx=6, D=8)
    ctx.sync()
    assert (T.cpu().numpy() == 7.0).all()                 # the outputs are left alone
    upd = "bsc_glm_scalar_hier_update"
    with pytest.raises(BayesicHipError, match=upd + ": stats is null"):
        ctx.call(upd, None, ell, G, ell, G, ell, W, Bz, lt, 8, 3, 8, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1, 0.01, 0.9, 0.999,
                 1e-8, 1, 1, None, 1, None, None, None, ell, G)
    with pytest.raises(BayesicHipError, match=upd + ": group_a0=0 group_b0=1 must be positive"):
        ctx.call(upd, ell, ell, G, ell, G, ell, W, Bz, lt, 8, 3, 8, 1.0, 1.0, 1.0, 1.0, 0.0, 1.0, 1, 0.01, 0.9, 0.999,
                 1e-8, 1, 1, None, 1, None, None, None, ell, G)
    with pytest.raises(BayesicHipError, match=upd + ": next-draw buffers must be all set or all null"):
        ctx.call(upd, ell, ell, G, ell, G, ell, W, Bz, lt, 8, 3, 8, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1, 0.01, 0.9, 0.999,
                 1e-8, 1, 1, None, 1, None, None, lt[8:], ell, G)
    ctx.sync()


# ---- the finish -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ready", [1, 0])
@pytest.mark.parametrize("S", [1, 8, 11])
@pytest.mark.parametrize("J", [1, 3, 1000])
def test_finish_from_given_statistics(ctx, J, S, ready):
    """bsc_glm_scalar_hier_update(stats): float64 on both sides."""
    D = 24
    P = D + J + 2
    rs = np.random.RandomState(J + S)
    f64 = torch.float64
    lam = np.concatenate([0.2 * rs.standard_normal(P), math.log(0.1) + 0.1 * rs.standard_normal(P)])
    m1, m2 = 0.01 * rs.standard_normal(2 * P), 1e-4 * rs.uniform(size=2 * P)
    ell, G, H = -100.0 * rs.uniform(1, 2, S), rs.standard_normal((S, D)) * 5, rs.standard_normal((S, J)) * 3
    T = rs.standard_normal(S) * 7
    seed, t, scale, prec, a0, b0, ga0, gb0, lr = 99, 4, 12.5, 0.7, 1.5, 0.8, 1.3, 0.6, 0.02
    eps, eps_n = ref.noise(D, J, S, seed, t - 1), ref.noise(D, J, S, seed, t)
    W, Bm, zeta, logtau = ref.draw(lam, eps, D, J)
    n_bz = ((S + 7) // 8) * J * 8
    d = dict(stats=ctx.to_device(np.concatenate([ell, G.ravel(), H.ravel(), T]), f64), lam=ctx.to_device(lam, f64),
             out=ctx.zeros(2 * P, f64), m1=ctx.to_device(m1, f64), m2=ctx.to_device(m2, f64),
             eps=ctx.to_device(eps.ravel(), f64), W=ctx.to_device(W.ravel()), Bz=ctx.to_device(ref.chunked(Bm)),
             lt=_dev_vec(ctx, logtau),
             eps_n=ctx.to_device(eps_n.ravel() if ready else np.zeros(S * P), f64), W_n=ctx.zeros(S * D),
             Bz_n=torch.full((n_bz,), 5.0, dtype=torch.float32, device=ctx.device),
             lt_n=torch.full((S + 4,), 5.0, dtype=torch.float32, device=ctx.device), elbo=ctx.zeros(1, f64),
             grad=ctx.zeros(2 * P, f64))
    ctx.call("bsc_glm_scalar_hier_update", d["stats"], d["lam"], d["out"], d["m1"], d["m2"], d["eps"], d["W"], d["Bz"],
             d["lt"], D, J, S, scale, prec, a0, b0, ga0, gb0, t, lr, 0.9, 0.999, 1e-8, seed, t, d["eps_n"], ready,
             d["W_n"], d["Bz_n"], d["lt_n"], d["elbo"], d["grad"])
    ctx.sync()
    lam_r, m1_r, m2_r, elbo_r, grad_r = ref.finish(lam, m1, m2, t, eps, W, Bm, zeta, logtau, ell, G, H, T, scale, prec,
                                                   a0, b0, ga0, gb0, lr)
    npt.assert_allclose(d["elbo"].item(), elbo_r, rtol=1e-9)
    npt.assert_allclose(d["grad"].cpu().numpy(), grad_r, rtol=1e-9, atol=1e-9 * np.abs(grad_r).max())
    npt.assert_allclose(d["out"].cpu().numpy(), lam_r, rtol=1e-9, atol=1e-12)
    npt.assert_allclose(d["m1"].cpu().numpy(), m1_r, rtol=1e-9, atol=1e-15)
    npt.assert_allclose(d["m2"].cpu().numpy(), m2_r, rtol=1e-9, atol=1e-18)
    npt.assert_allclose(d["lam"].cpu().numpy(), lam, rtol=0, atol=0)       # lam_in is not modified
    npt.assert_allclose(d["eps_n"].cpu().numpy().reshape(S, P), eps_n, rtol=1e-12, atol=1e-14)
    # the next draws: float32-rounded from float64 on both sides (1 ulp where the float64 values straddle a tie)
    W_r, Bm_r, _, lt_r = ref.draw(lam_r, eps_n, D, J)
    npt.assert_allclose(d["W_n"].cpu().numpy().reshape(S, D), W_r, rtol=2e-7, atol=1e-9)
    Bz_n = d["Bz_n"].cpu().numpy()
    npt.assert_allclose(ref.unchunk(Bz_n, S, J), Bm_r, rtol=2e-7, atol=1e-9)
    assert (Bz_n.reshape(-1, J, 8)[-1][:, S - 8 * ((S - 1) // 8):] == 0.0).all()      # the dead slots are zeroed
    lt_n = d["lt_n"].cpu().numpy()
    npt.assert_allclose(lt_n[:S], lt_r, rtol=2e-7, atol=1e-9)
    assert (lt_n[S:] == 5.0).all()                        # nothing behind logtau_next [S] is written


# ---- the drivers ----------------------------------------------------------------------------------------------------

def _hierarchy(fam, B, D, J, seed):
    """Grouped regression data with offsets and weights; weibull: (X, time, event, g, o, v), else (X, y, g, o, v).
    negbin: tests/test_glm_nb_gpu.py's low-mean counts (offsets moved by -1.5, phi = 2: rates below one event per row),
    so that the ELBO is of the size of its terms and a relative tolerance on it is a statement about the pass."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    o = (0.5 * rs.standard_normal(B) + (-1.5 if fam == "negbin" else 0.0)).astype(np.float32)
    v = rs.uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    L = X.astype(np.float64) @ rs.standard_normal(D) + 0.7 * rs.standard_normal(J)[g] + o
    if fam == "negbin":
        return X, rs.negative_binomial(2.0, 2.0 / (2.0 + np.exp(L))).astype(np.float32), g, o, v
    L = np.minimum(L, 3.0)
    if fam == "gamma":
        return X, np.maximum(rs.gamma(2.0, np.exp(L) / 2.0), 1e-30).astype(np.float32), g, o, v
    t = np.maximum(np.exp(L) * rs.weibull(1.5, B), 1e-30)
    ev = rs.uniform(size=B) >= 0.3
    return X, np.where(ev, t, t * rs.uniform(0.1, 1.0, B)).astype(np.float32), ev, g, o, v


def _make(fam, ctx, dev, J, **kw):
    from bayesic_amd.svi import HierGammaReparamSVI, HierNegBinReparamSVI, HierWeibullReparamSVI
    if fam == "weibull":
        X, t, ev, g, o, v = dev
        return HierWeibullReparamSVI(X, t, g, J, event=ev, offset=o, weights=v, ctx=ctx, **kw)
    X, y, g, o, v = dev
    cls = HierNegBinReparamSVI if fam == "negbin" else HierGammaReparamSVI
    return cls(X, y, g, J, offset=o, weights=v, ctx=ctx, **kw)


def _set(fam, model, dev):
    if fam == "weibull":
        X, t, ev, g, o, v = dev
        model.set_batch(X, t, event=ev, offset=o, weights=v, groups=g)
    else:
        X, y, g, o, v = dev
        model.set_batch(X, y, offset=o, weights=v, groups=g)


def _host(fam, b):
    """(X, y signed, g, o, v) of a _hierarchy batch."""
    if fam == "weibull":
        X, t, ev, g, o, v = b
        return X, np.where(ev, t, -t).astype(np.float32), g, o, v
    return b


@pytest.mark.parametrize("S", [8, 11])
@pytest.mark.parametrize("fam", FAMILIES)
def test_twenty_updates_track_the_reference_over_two_batches(ctx, fam, S):
    """set_batch with new rows, new groups, new offsets and weights before every update.  The ELBO is held to each
    family's own criterion.  negbin: tests/test_glm_nb_gpu.py's -- rtol 1e-6 of the ELBO itself, on low-mean counts for
    which the condition number (the size of the data terms over |ELBO|, from reference quantities alone) is asserted to
    stay below 4.  gamma and weibull: within 1e-6 of the size of the data terms, scale * mean_s b_ell[s]; their own tests
    allow 1e-6 of a larger size that also counts the prior's terms."""
    B, D, J, seed, lr, prec, a0, b0, ga0, gb0 = 1029, 256, 20, 1234, 0.01, 2.0, 1.5, 0.5, 1.5, 0.8
    batches = [_hierarchy(fam, B, D, J, 10 + k) for k in range(2)]
    dev = [tuple(ctx.to_device(a) for a in b) for b in batches]
    model = _make(fam, ctx, dev[0], J, n_total=10.0 * B, n_samples=S, seed=seed, lr=lr, prior_precision=prec, a0=a0,
                  b0=b0, group_a0=ga0, group_b0=gb0)
    P = D + J + 2
    lam = ref.init_lam(P)
    npt.assert_array_equal(model.lam.cpu().numpy(), lam)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    calls = []
    real_call = ctx.call
    ctx.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        for t in range(1, 21):
            k = (t - 1) % 2
            _set(fam, model, dev[k])
            assert model.step() is None
            Xh, yh, gh, oh, vh = _host(fam, batches[k])
            info = {}
            lam, m1, m2, elbo, grad = ref.step(fam, lam, m1, m2, t, Xh, yh, gh, J, S, seed, 10.0 * B, lr, prec, a0, b0,
                                               ga0, gb0, offset=oh, weights=vh, info=info)
            if t in (1, 2, 3, 10, 20):
                ctx.sync()
                gd = model.grad.cpu().numpy()
                e = abs(model.elbo.item() - elbo)
                print("%s t=%d: ELBO %.6g, error %.3g of the data terms' size %.6g; grad err/max %.3g; lam err %.3g" % (
                    fam, t, elbo, e / info["size"], info["size"], np.abs(gd - grad).max() / np.abs(grad).max(),
                    np.abs(model.lam.cpu().numpy() - lam).max()))
                if fam == "negbin":
                    assert info["size"] <= 4.0 * abs(elbo), info["size"] / abs(elbo)
                    npt.assert_allclose(model.elbo.item(), elbo, rtol=1e-6)
                else:
                    assert e <= 1e-6 * info["size"], (e, info["size"])
                assert np.abs(gd - grad).max() <= 1e-4 * np.abs(grad).max()
                npt.assert_allclose(model.lam.cpu().numpy(), lam, atol=2e-4)
    finally:
        ctx.call = real_call
    assert "bsc_glm_scalar_data_pass_groups" in calls and "bsc_glm_scalar_hier_update" in calls
    assert not [c for c in calls if c.startswith("bsc_glm_") and "_scalar_" not in c and "group_plan" not in c]
    p = model.params()
    npt.assert_allclose(np.concatenate([p["m"], p["rho"]]), lam, atol=2e-4)
    assert p["w"][0].shape == (D,) and p["b"][1].shape == (J,)
    npt.assert_array_equal(p["b"][0], p["m"][D:D + J])
    assert p["zeta"][0] == p["m"][P - 2] and p["tau"][1] == p["rho"][P - 1]
    key = "phi_mean" if fam == "negbin" else "shape_mean"
    npt.assert_allclose(p[key], math.exp(lam[P - 1] + 0.5 * math.exp(2.0 * lam[2 * P - 1])), rtol=1e-3)


def test_set_batch_and_refusals_of_the_drivers(ctx):
    from bayesic_amd._ffi import BayesicHipError
    from bayesic_amd.svi import HierNegBinReparamSVI, HierWeibullReparamSVI
    B, D, J = 325, 64, 5
    X, y, g, o, v = _hierarchy("negbin", B, D, J, 7)
    Xd, yd, gd = ctx.to_device(X), ctx.to_device(y), ctx.to_device(g)
    a = HierNegBinReparamSVI(Xd, yd, gd, J, n_samples=8, seed=3, ctx=ctx)
    b = HierNegBinReparamSVI(Xd, yd, g, J, n_samples=8, seed=3, ctx=ctx)              # host ids are uploaded
    b.set_batch(Xd.data_ptr(), yd.data_ptr(), rows=B, groups=gd.data_ptr())          # raw pointers are taken as they are
    c = HierNegBinReparamSVI(Xd, yd, gd, J, n_samples=8, seed=3, ctx=ctx)
    plan = c.build_plan(gd, B)                                                       # built once, outside the loop
    assert plan[1] == a.n_segments
    npt.assert_array_equal(plan[0].cpu().numpy(), a.plan.cpu().numpy())
    c.set_batch(Xd, yd, groups=gd, plan=plan)
    assert c.plan is plan[0]                                                         # taken, not rebuilt
    for m in (a, b, c):
        m.step()
        m.step()
    ctx.sync()
    npt.assert_array_equal(a.lam.cpu().numpy(), b.lam.cpu().numpy())
    npt.assert_array_equal(a.lam.cpu().numpy(), c.lam.cpu().numpy())
    assert a.n_segments == len(np.unique(g))
    with pytest.raises(ValueError, match="set_batch needs groups="):
        a.set_batch(Xd, yd)
    bad = g.copy()
    bad[17] = J
    with pytest.raises(BayesicHipError, match=r"row 17 has group id 5 outside \[0,5\)"):
        a.set_batch(Xd, yd, groups=ctx.to_device(bad))
    with pytest.raises(ValueError, match="finite and >= 0"):
        a.set_batch(Xd, -yd - 1.0, groups=gd)
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        a.predict(Xd)
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        a.heldout_lpd(Xd, yd)
    w = HierWeibullReparamSVI(Xd, yd + 1.0, gd, J, ctx=ctx)
    with pytest.raises(NotImplementedError, match="not built"):
        w.set_batch(Xd, yd + 1.0, groups=gd, upper=yd + 2.0)
    with pytest.raises(ValueError, match="time must be finite and > 0"):
        w.set_batch(Xd, yd, groups=gd)
