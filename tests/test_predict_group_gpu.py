"""GPU parity of the grouped posterior predictive (csrc/bsc_predict_group.hip through the C ABI, svi/predict.py,
svi/hier_glm.py and the plugin route) against the float64 restatement in tests/_predict_group_ref.py.

    l[n,s] = x_n . w_s + Bt[row(g_n), s] + o_n,      row(-1) = J, row(j) = j

Bounds are tests/test_predict_gpu.py's (float64 reference quantities and the project's factor 2e-5) with the magnitude
term a_ns = sum_d |x_nd w_sd| + |b_s[g_n]| + |o_n|: the intercept and the offset are two more float32 additions to l.
tests/test_predict_group_cpu.py holds a float32 evaluation of the reference inside these bounds at the shapes used here.
Poisson inputs keep |l| <= 4 (asserted on the float64 logits), as tests/test_predict_gpu.py's do.

Shapes: D in {4, 64, 132, 256} is one strip, one strip, two strips of the general kernel, and the FULL kernel; S in
{1, 8, 16, 17, 33, 64} is every chunk count (1, 2, 4), the empty chunk (33) and the masked tail; B in {1, 15, 16, 17,
325} is one ragged tile, a full one, two, and several waves; J in {1, 5, 1000}.  Batches where a wave runs two and
three tiles are sized from the device's CU count as tests/test_regression_multi_tile_gpu.py sizes them.

Measured on an MI355X (256 CUs), worst error / bound over the parity product: mean 0.007, var 0.010, lpd 0.031,
lpd_sum 0.011; the exact-accounting and zero-table cases hold bit for bit; end to end the held-out log density per row
is -0.4998 with the true ids against -0.6953 with every row marked -1 (logistic), -1.4055 against -2.1394 (Poisson),
equal to the float64 fit of the same run to the digits shown."""
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_group_ref as grp
import _predict_group_ref as ref
import _predict_ref as pref

pytestmark = pytest.mark.gpu

FAMILIES = ref.FAMILIES
SENTINEL = -777.0
GUARD = 64                            # sentinel elements past B
NAMES = ("mean", "var", "lpd", "lpd_sum")
FAR_ID = 1 << 20                      # an id far outside every table used here


# ---- helpers ----------------------------------------------------------------------------------------------------------

def _upload(ctx, X, y, g, W, Bt, offset=None, ld=None, g_shift=False, guard=0):
    """Device operands.  ``guard`` rows of NaN (X, y, offset) and of FAR_ID (groups) follow the batch; ``g_shift`` puts
    the ids at a 4-byte-but-not-16-byte aligned address."""
    B, D = X.shape
    buf = np.full((B + guard, ld or D), np.nan if guard else 7.0, np.float32)
    buf[:B, :D] = X
    if ld is not None and guard:
        buf[:B, D:] = 7.0
    tail = np.full(guard, np.nan, np.float32)
    d = dict(X=ctx.to_device(buf), W=ctx.to_device(W), Bt=ctx.to_device(Bt), y=None, o=None)
    if y is not None:
        d["y"] = ctx.to_device(np.concatenate([y, tail]).astype(np.float32))
    if offset is not None:
        d["o"] = ctx.to_device(np.concatenate([offset, tail]).astype(np.float32))
    ids = np.concatenate([[FAR_ID] if g_shift else [], g, np.full(guard, FAR_ID)]).astype(np.int32)
    d["g"] = ctx.to_device(ids)[1:] if g_shift else ctx.to_device(ids)
    if g_shift:
        assert d["g"].data_ptr() % 16 == 4
    return d


def _launch(ctx, family, d, B, D, J, S, ld=None, want=NAMES, guard=0, entry="groups"):
    out = {k: torch.full((B + guard,), SENTINEL, dtype=torch.float32, device=ctx.device) for k in NAMES[:3]}
    out["lpd_sum"] = torch.full((1,), SENTINEL, dtype=torch.float64, device=ctx.device)
    args = [out[k] if k in want else None for k in NAMES]
    if entry == "groups":
        ctx.call("bsc_predict_pass_groups", ref.CODE[family], d["X"], ld or D, d["y"], d["o"], d["g"], B, D, J, d["W"],
                 d["Bt"], int(d["Bt"].stride(0)), S, *args)
    else:
        ctx.call("bsc_predict_pass_offset", ref.CODE[family], d["X"], ld or D, d["y"], d["o"], B, D, d["W"], None, S,
                 *args)
    ctx.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(ctx, family, X, y, g, W, Bt, offset=None, ld=None, want=NAMES, g_shift=False, guard=0):
    """bsc_predict_pass_groups on host arrays; outputs not in ``want`` are passed as NULL.  Dict of numpy arrays, each
    per-row one ``guard`` elements longer than B."""
    d = _upload(ctx, X, y, g, W, Bt, offset, ld, g_shift, guard)
    return _launch(ctx, family, d, X.shape[0], X.shape[1], Bt.shape[0] - 1, W.shape[0], ld, want, guard)


def _inputs(family, B, D, J, S, seed, with_offset=True):
    """tests/test_glm_group_gpu._inputs' recipe with ids in [-1, J) and the table of _predict_group_ref."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    b = (0.5 * rs.standard_normal((S, J))).astype(np.float32)
    b_new = (0.8 * rs.standard_normal(S)).astype(np.float32)
    g = rs.randint(-1, J, size=B).astype(np.int32)
    o = rs.standard_normal(B).astype(np.float32) if with_offset else None
    if family == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, g, W, ref.table(b, b_new), o)).max()
        if peak > 3.5:
            W, b, b_new = ((a * (3.5 / peak)).astype(np.float32) for a in (W, b, b_new))
            o = None if o is None else (o * (3.5 / peak)).astype(np.float32)
    return X, y, g, W, ref.table(b, b_new), o


def _assert_inside(family, got, X, y, g, W, Bt, o, what=""):
    """Every output, every row, inside _predict_group_ref.bounds; returns the worst error / bound per output."""
    B = X.shape[0]
    want = ref.predict(family, X, g, W, Bt, y, o)
    bnd = ref.bounds(family, X, g, W, Bt, y, o)
    if family == "poisson":
        assert np.abs(ref.logits(X, g, W, Bt, o)).max() <= 4.0
    worst = {}
    for k in NAMES:
        err = np.abs(got[k][:B] - want[k]) if k != "lpd_sum" else np.abs(got[k] - want[k])
        worst[k] = float(np.max(err / (bnd[k] + 1e-300)))
    for k, w in worst.items():
        assert w <= 1.0, (what, k, w)
    return worst


def _check(ctx, family, X, y, g, W, Bt, o, **kw):
    got = _run(ctx, family, X, y, g, W, Bt, o, **kw)
    return got, _assert_inside(family, got, X, y, g, W, Bt, o)


def _n_iter(B, cu):
    """predict_setup's arithmetic (csrc/bsc_predict_pass.h): eight waves per workgroup, one workgroup per CU."""
    n_tiles = (B + 15) // 16
    return (n_tiles + 8 * cu - 1) // (8 * cu)


def _rows_for(n_iter, cu):
    """A batch whose waves run n_iter tiles: n_iter - 1 full sweeps, one full tile and a ragged one of five rows."""
    return (n_iter - 1) * 8 * cu * 16 + 16 + 5


# ---- 1. parity ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [4, 64, 132, 256])
@pytest.mark.parametrize("family", FAMILIES)
def test_pass_matches_the_reference(ctx, family, D):
    worst = dict.fromkeys(NAMES, 0.0)
    for S in (1, 8, 16, 17, 33, 64):
        for B in (1, 15, 16, 17, 325):
            for J in (1, 5, 1000):
                for with_offset in (False, True):
                    X, y, g, W, Bt, o = _inputs(family, B, D, J, S, seed=B * 7 + D + S + J, with_offset=with_offset)
                    assert Bt.shape == (J + 1, ref.table_ld(S))
                    got = _run(ctx, family, X, y, g, W, Bt, o)
                    w = _assert_inside(family, got, X, y, g, W, Bt, o, what=(S, B, J, with_offset))
                    worst = {k: max(worst[k], w[k]) for k in NAMES}
    print("%s D=%d: worst error / bound  mean %.3g  var %.3g  lpd %.3g  lpd_sum %.3g" % (
        family, D, worst["mean"], worst["var"], worst["lpd"], worst["lpd_sum"]))


@pytest.mark.parametrize("B,D,ld", [(333, 64, 96), (325, 256, 260), (50, 132, 512)])
@pytest.mark.parametrize("family", FAMILIES)
def test_pass_respects_the_leading_dimensions(ctx, family, B, D, ld):
    X, y, g, W, Bt, o = _inputs(family, B, D, 5, 17, seed=ld)
    got, _ = _check(ctx, family, X, y, g, W, Bt, o, ld=ld)
    wide = np.full((Bt.shape[0], Bt.shape[1] + 12), 5.0, np.float32)       # ldb = 44: past S, not a whole chunk
    wide[:, :17] = Bt[:, :17]
    d = _upload(ctx, X, y, g, W, wide, o, ld=ld)
    again = _launch(ctx, family, d, B, D, 5, 17, ld=ld)
    for k in NAMES:
        npt.assert_array_equal(again[k], got[k])


@pytest.mark.parametrize("family", FAMILIES)
def test_ids_that_are_not_16_byte_aligned(ctx, family):
    X, y, g, W, Bt, o = _inputs(family, 325, 256, 5, 8, seed=3)
    _check(ctx, family, X, y, g, W, Bt, o, g_shift=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_each_output_is_optional_and_the_others_do_not_change(ctx, family):
    X, y, g, W, Bt, o = _inputs(family, 325, 132, 5, 16, seed=8)
    full = _run(ctx, family, X, y, g, W, Bt, o)
    for drop in NAMES:
        got = _run(ctx, family, X, y, g, W, Bt, o, want=tuple(k for k in NAMES if k != drop))
        assert (got[drop] == SENTINEL).all()
        for k in NAMES:
            if k != drop:
                npt.assert_array_equal(got[k], full[k])
    nol = _run(ctx, family, X, None, g, W, Bt, o, want=("mean", "var"))     # no y at all
    npt.assert_array_equal(nol["mean"], full["mean"])
    npt.assert_array_equal(nol["var"], full["var"])


# ---- 2. several tiles per wave ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [2, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_several_tiles_per_wave(ctx, family, n_iter):
    cu = int(ctx.info()["cu_count"])
    B, D, J, S = _rows_for(n_iter, cu), 8, 5, 17
    assert _n_iter(B, cu) == n_iter
    X, y, g, W, Bt, o = _inputs(family, B, D, J, S, seed=n_iter)
    got = _run(ctx, family, X, y, g, W, Bt, o, guard=GUARD)
    _assert_inside(family, got, X, y, g, W, Bt, o)
    for k in NAMES[:3]:
        assert (got[k][B:] == SENTINEL).all(), k


# ---- 3. exact row -> group -> draw accounting ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_iter", [1, 3])
def test_exact_row_group_draw_accounting(ctx, n_iter):
    """X = 0, W = 0, Poisson: mu = exp(Bt[row(g_n), s]) is exactly 1 where the table holds 0 and exactly 0 where it holds
    -200 (expf(-200) is 0 in float32), so the mean of a row is (number of zero draws of its group) / S without rounding:
    a wrong row, group or draw shows as a wrong bit."""
    cu = int(ctx.info()["cu_count"])
    B, D, J = (325 if n_iter == 1 else _rows_for(n_iter, cu)), 4, 5
    assert _n_iter(B, cu) == n_iter
    g = ((np.arange(B) * 7 + np.arange(B) // 16) % (J + 1) - 1).astype(np.int32)          # -1 .. J - 1, every tile mixed
    X = np.zeros((B, D), np.float32)
    for S in (17, 64):
        W = np.zeros((S, D), np.float32)
        d = _upload(ctx, X, None, g, W, np.zeros((J + 1, ref.table_ld(S)), np.float32), guard=GUARD)
        for j0 in (0, J - 1, J):
            hit = ref.rows_of(g, J) == j0
            assert hit.any() and not hit.all()
            for s0 in (None, 0, 3, 4, 15, 16, S - 1):
                Bt = np.full((J + 1, ref.table_ld(S)), -200.0, np.float32)
                Bt[:, S:] = 0.0
                if s0 is None:
                    Bt[j0, :S] = 0.0
                    expect = np.float32(1.0)
                else:
                    Bt[j0, s0] = 0.0
                    expect = np.float32(1.0) / np.float32(S)
                d["Bt"].copy_(torch.from_numpy(Bt))
                got = _launch(ctx, "poisson", d, B, D, J, S, want=("mean",), guard=GUARD)["mean"]
                npt.assert_array_equal(got[:B], np.where(hit, expect, np.float32(0.0)), err_msg=str((S, j0, s0)))
                assert (got[B:] == SENTINEL).all()


# ---- 4. identities ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D,S", [(64, 8), (132, 17), (256, 64)])
@pytest.mark.parametrize("family", FAMILIES)
def test_a_zero_table_is_the_offset_pass_bit_for_bit(ctx, family, D, S):
    X, y, g, W, Bt, o = _inputs(family, 325, D, 5, S, seed=D)
    d = _upload(ctx, X, y, g, W, np.zeros_like(Bt), o)
    a = _launch(ctx, family, d, 325, D, 5, S)
    b = _launch(ctx, family, d, 325, D, 5, S, entry="offset")
    for k in NAMES:
        npt.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("family", FAMILIES)
def test_the_one_hot_design_through_the_shipped_pass_agrees(ctx, family):
    """[X | onehot(row(g))] against [W | b | b_new] is the same model: D + J + 1 = 12 columns."""
    B, D, J, S = 325, 8, 3, 17
    X, y, g, W, Bt, _ = _inputs(family, B, D, J, S, seed=5, with_offset=False)
    got = _run(ctx, family, X, y, g, W, Bt)
    X1 = np.concatenate([X, grp.onehot(ref.rows_of(g, J), J + 1)], axis=1)
    W1 = np.concatenate([W, Bt[:, :S].T], axis=1).astype(np.float32)
    out = {k: torch.full((B,), SENTINEL, dtype=torch.float32, device=ctx.device) for k in NAMES[:3]}
    out["lpd_sum"] = torch.full((1,), SENTINEL, dtype=torch.float64, device=ctx.device)
    ctx.call("bsc_predict_pass", ref.CODE[family], ctx.to_device(X1), D + J + 1, ctx.to_device(y), B, D + J + 1,
             ctx.to_device(W1), None, S, *[out[k] for k in NAMES])
    ctx.sync()
    b0, b1 = ref.bounds(family, X, g, W, Bt, y), pref.bounds(family, X1, W1, None, y)
    for k in NAMES:
        assert (np.abs(got[k] - out[k].cpu().numpy()) <= b0[k] + b1[k]).all(), k


# ---- 5. extremes ------------------------------------------------------------------------------------------------------

def test_logistic_at_extreme_logits_through_the_intercept(ctx):
    B, D, J, S = 200, 256, 3, 8
    X, W = np.zeros((B, D), np.float32), np.zeros((S, D), np.float32)
    Bt = np.zeros((J + 1, 16), np.float32)
    Bt[0, :S], Bt[1, :S], Bt[J, :S] = 80.0, -80.0, -80.0
    g = (np.arange(B) % (J + 1) - 1).astype(np.int32)
    y = ((np.arange(B) // (J + 1)) % 2).astype(np.float32)
    got = _run(ctx, "logistic", X, y, g, W, Bt)
    L = ref.logits(X, g, W, Bt)
    assert set(np.unique(L)) == {-80.0, 0.0, 80.0} and len({(a, b) for a, b in zip(L[:, 0], y)}) == 6
    for k in NAMES:
        assert np.isfinite(got[k]).all(), k
    _assert_inside("logistic", got, X, y, g, W, Bt, None)


def test_poisson_at_its_largest_logit_through_the_intercept(ctx):
    """tests/test_predict_gpu.py holds the Poisson family to its bounds for |l| <= 4; here l = 4 is the intercept alone."""
    B, D, J, S = 200, 64, 3, 8
    X, W = np.zeros((B, D), np.float32), np.zeros((S, D), np.float32)
    Bt = np.zeros((J + 1, 16), np.float32)
    Bt[0, :S], Bt[1, :S], Bt[J, :S] = 4.0, -4.0, 4.0
    g = (np.arange(B) % (J + 1) - 1).astype(np.int32)
    y = (np.arange(B) % 7).astype(np.float32)
    got = _run(ctx, "poisson", X, y, g, W, Bt)
    assert np.abs(ref.logits(X, g, W, Bt)).max() == 4.0
    _assert_inside("poisson", got, X, y, g, W, Bt, None)


@pytest.mark.parametrize("S", [8, 33])
def test_every_draw_at_minus_infinity_gives_minus_infinity(ctx, S):
    B, D, J = 40, 8, 2
    X, W = np.zeros((B, D), np.float32), np.zeros((S, D), np.float32)
    Bt = np.zeros((J + 1, ref.table_ld(S)), np.float32)
    Bt[1, :S] = -np.inf
    g = (np.arange(B) % J).astype(np.int32)
    y = np.ones(B, np.float32)
    got = _run(ctx, "poisson", X, y, g, W, Bt, want=("mean", "var", "lpd"))
    gone = g == 1
    assert (got["lpd"][gone] == -np.inf).all() and (got["mean"][gone] == 0.0).all()
    npt.assert_allclose(got["lpd"][~gone], -1.0, rtol=1e-6)


# ---- 6. determinism ---------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_identical(ctx):
    cu = int(ctx.info()["cu_count"])
    X, y, g, W, Bt, o = _inputs("poisson", _rows_for(2, cu), 8, 1000, 33, seed=1)
    d = _upload(ctx, X, y, g, W, Bt, o)
    a, b = (_launch(ctx, "poisson", d, X.shape[0], 8, 1000, 33) for _ in range(2))
    for k in NAMES:
        npt.assert_array_equal(a[k], b[k])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------

def test_refusals_name_the_quantity_and_leave_the_outputs_alone(ctx):
    from bayesic_amd._ffi import BayesicHipError
    dev = ctx.device
    Xb = torch.zeros((9, 256), dtype=torch.float32, device=dev)
    Wb = torch.zeros((65 * 256,), dtype=torch.float32, device=dev)
    Btb = torch.zeros((6 * 68 + 4,), dtype=torch.float32, device=dev)
    y, gd = torch.zeros(9, dtype=torch.float32, device=dev), torch.zeros(9, dtype=torch.int32, device=dev)
    out = [torch.full((9,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    out.append(torch.full((1,), SENTINEL, dtype=torch.float64, device=dev))

    def call(match, family=1, D=256, J=5, Bt=Btb, ldb=16, S=8, g=gd):
        with pytest.raises(BayesicHipError, match=match) as e:
            ctx.call("bsc_predict_pass_groups", family, Xb, 256, y, None, g, 9, D, J, Wb, Bt, ldb, S, *out)
        assert "status -3:" in str(e.value), str(e.value)          # BSC_ERR_UNSUPPORTED
        ctx.sync()
        for o in out:
            assert (o.cpu().numpy() == SENTINEL).all()

    call("family=0", family=0)
    call("J=0", J=0)
    call("J=65537", J=65537)
    call("ldb=4", ldb=4)
    call("ldb=18", ldb=18)
    call("Bt must be 16-byte aligned", Bt=Btb[1:])
    call("groups and Bt must not be null", g=None)
    call("S=65", S=65, ldb=68)
    call("D=6", D=6)
    # the next valid call is right
    X, yv, g, W, Bt, o = _inputs("logistic", 9, 256, 5, 8, seed=2)
    _check(ctx, "logistic", X, yv, g, W, Bt, o)


def test_the_id_check_names_row_and_id(ctx):
    from bayesic_amd._ffi import BayesicHipError
    J, B = 5, 5000
    g = (np.arange(B) % J).astype(np.int32)
    g[3] = -1
    gd = ctx.to_device(g)
    ctx.call("bsc_group_ids_check", gd, B, J, 1)
    with pytest.raises(BayesicHipError, match=r"row 3 has group id -1 outside \[0,5\)"):
        ctx.call("bsc_group_ids_check", gd, B, J, 0)
    for bad, said in ((J, r"row 4321 has group id 5 outside \[-1,5\)"), (-2, r"row 4321 has group id -2 outside \[-1,5\)")):
        h = g.copy()
        h[4321], h[4700] = bad, bad                      # the first offending row is the one named
        with pytest.raises(BayesicHipError, match=said):
            ctx.call("bsc_group_ids_check", ctx.to_device(h), B, J, 1)
    ctx.call("bsc_group_ids_check", gd, 0, J, 0)        # an empty batch has no offending row


# ---- 8. drivers -------------------------------------------------------------------------------------------------------

def _hierarchy(link, B, D, J, seed, sd=2.0):
    """tests/test_glm_group_gpu._hierarchy's data with strong group intercepts."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    o = (0.3 * rs.standard_normal(B)).astype(np.float32)
    L = X.astype(np.float64) @ rs.standard_normal(D) + sd * np.linspace(-1.0, 1.0, J)[g] + o
    if link == "logistic":
        y = (rs.uniform(size=B) < 1.0 / (1.0 + np.exp(-L))).astype(np.float32)
    else:
        y = rs.poisson(np.exp(np.minimum(L, 3.0))).astype(np.float32)
    return X, y, g, o


def _as_numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("link", FAMILIES)
def test_driver_predict_is_the_reference_at_its_own_draws(ctx, link):
    from bayesic_amd.svi import HierGLMReparamSVI, predict as mod
    B, D, J = 300, 8, 5
    X, y, g, o = _hierarchy(link, B, D, J, 3, sd=1.0)
    m = HierGLMReparamSVI(X, y, g, J, link=link, n_samples=8, seed=9, lr=0.05, offset=o, ctx=ctx)
    for _ in range(3):
        m.step()
    ctx.sync()
    lam = m.lam.cpu().numpy()
    g2 = g.copy()
    g2[::4] = -1
    for S, seed in ((64, None), (17, 77)):
        W, Bt = mod.posterior_draws(m, S, seed)
        W_r, Bt_r = ref.posterior_draws(lam, D, J, S, m.seed if seed is None else seed)
        assert tuple(Bt.shape) == (J + 1, ref.table_ld(S)) and Bt.stride(0) == ref.table_ld(S)
        npt.assert_array_equal(W.cpu().numpy(), W_r)
        npt.assert_allclose(Bt.cpu().numpy(), Bt_r, rtol=1e-6)            # (bitwise up to libm's exp)
        assert (Bt.cpu().numpy()[:, S:] == 0).all()
        out = _as_numpy(m.predict(X, y, groups=g2, n_samples=S, seed=seed, offset=o))
        direct = _run(ctx, link, X, y, g2, W.cpu().numpy(), Bt.cpu().numpy(), o)
        for k in NAMES:
            npt.assert_array_equal(out[k], direct[k])
        _assert_inside(link, out, X, y, g2, W.cpu().numpy(), Bt.cpu().numpy(), o)
        assert m.heldout_lpd(X, y, groups=g2, n_samples=S, seed=seed, offset=o) == direct["lpd_sum"][0] / B
    # draws= reused across calls, the ids as a device tensor and as a raw pointer
    draws = mod.posterior_draws(m, 16, 5)
    gd = ctx.to_device(g2)
    a = _as_numpy(m.predict(X, y, groups=gd, draws=draws, offset=o))
    b = _as_numpy(m.predict(X, y, groups=int(gd.data_ptr()), draws=draws, offset=o))
    c = _as_numpy(m.predict(X, y, groups=g2, n_samples=16, seed=5, offset=o))
    for k in NAMES:
        npt.assert_array_equal(a[k], b[k])
        npt.assert_array_equal(a[k], c[k])
    # weights: per-row outputs unchanged, the weighted sum and the weights' sum
    v = np.random.RandomState(1).uniform(0.0, 2.0, B).astype(np.float32)
    v[::6] = 0.0
    w = _as_numpy(m.predict(X, y, groups=gd, draws=draws, offset=o, weights=v))
    npt.assert_array_equal(w["lpd"], a["lpd"])
    npt.assert_allclose(w["lpd_sum"][0], (v.astype(np.float64) * a["lpd"].astype(np.float64)).sum(), rtol=1e-12)
    npt.assert_allclose(w["weight_sum"][0], v.astype(np.float64).sum(), rtol=1e-12)
    assert m.heldout_lpd(X, y, groups=gd, draws=draws, offset=o, weights=v) == w["lpd_sum"][0] / w["weight_sum"][0]
    # refusals of the Python layer
    from bayesic_amd._ffi import BayesicHipError
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y, groups=gd)
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        m.predict(X, y, offset=o)
    bad = g2.copy()
    bad[17] = J
    with pytest.raises(BayesicHipError, match=r"row 17 has group id 5 outside \[-1,5\)"):
        m.predict(X, y, groups=bad, offset=o)
    with pytest.raises(TypeError, match="int32"):
        m.predict(X, y, groups=gd.to(torch.int64), offset=o)
    with pytest.raises(ValueError, match=r"contiguous \[300\]"):
        m.predict(X, y, groups=gd[:-1], offset=o)


def test_a_model_fitted_with_exposure_refuses_to_predict_without_one(ctx):
    from bayesic_amd.svi import HierGLMReparamSVI
    B, D, J = 64, 8, 3
    X, y, g, o = _hierarchy("poisson", B, D, J, 4, sd=0.5)
    m = HierGLMReparamSVI(X, y, g, J, link="poisson", exposure=np.exp(o), ctx=ctx)
    with pytest.raises(ValueError, match="fitted with an offset"):
        m.predict(X, y, groups=g)
    a = _as_numpy(m.predict(X, y, groups=g, exposure=np.exp(o)))
    b = _as_numpy(m.predict(X, y, groups=g, offset=np.log(np.exp(o))))
    npt.assert_allclose(a["mean"], b["mean"], rtol=1e-5)


E2E = dict(B=600, D=8, J=5, steps=20, lr=0.1, seed=11)


def _e2e_data(link):
    X, y, g, o = _hierarchy(link, 2 * E2E["B"], E2E["D"], E2E["J"], 21)
    B = E2E["B"]
    return (X[:B], y[:B], g[:B], o[:B]), (X[B:], y[B:], g[B:], o[B:])


@pytest.mark.parametrize("link", FAMILIES)
def test_end_to_end_known_groups_beat_unseen_ones(ctx, link):
    """Twenty updates on data with strong group intercepts: held-out log density with the true ids is above that of the
    same rows marked -1, on the reference first (tests/test_predict_group_cpu.py runs the whole fit in float64)."""
    from bayesic_amd.svi import HierGLMReparamSVI, predict as mod
    (X, y, g, o), (Xt, yt, gt, ot) = _e2e_data(link)
    B, D, J = E2E["B"], E2E["D"], E2E["J"]
    m = HierGLMReparamSVI(X, y, g, J, link=link, n_samples=8, seed=E2E["seed"], lr=E2E["lr"], offset=o, ctx=ctx)
    for _ in range(E2E["steps"]):
        m.step()
    ctx.sync()
    W, Bt = ref.posterior_draws(m.lam.cpu().numpy(), D, J, 64, m.seed)
    new = np.full(B, -1, np.int32)
    r_known, r_new = ref.predict(link, Xt, gt, W, Bt, yt, ot), ref.predict(link, Xt, new, W, Bt, yt, ot)
    assert r_known["lpd_sum"] / B > r_new["lpd_sum"] / B + 0.02           # the reference itself orders them
    known = m.heldout_lpd(Xt, yt, groups=gt, offset=ot)
    unseen = m.heldout_lpd(Xt, yt, groups=new, offset=ot)
    print("%s held-out lpd per row: true ids %.4f (reference %.4f), every row a new group %.4f (reference %.4f)" % (
        link, known, r_known["lpd_sum"] / B, unseen, r_new["lpd_sum"] / B))
    assert known > unseen
    # the device's draws are the reference's (W bit for bit, Bt up to libm's exp); at ITS draws the reference bounds it
    Wd, Btd = (t.cpu().numpy() for t in mod.posterior_draws(m, 64))
    npt.assert_array_equal(Wd, W)
    npt.assert_allclose(Btd, Bt, rtol=1e-6)
    for got, ids in ((known, gt), (unseen, new)):
        want = ref.predict(link, Xt, ids, Wd, Btd, yt, ot)["lpd_sum"] / B
        assert abs(got - want) <= ref.bounds(link, Xt, ids, Wd, Btd, yt, ot)["lpd_sum"] / B


def test_the_plugin_route_predicts_through_the_driver(ctx):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    from bayesic_amd.inference import ReparamVI
    from bayesic_amd.svi import HierGLMReparamSVI
    from oracle import svi
    import test_glm_group_route_gpu as route_t
    N, D, G, S = 600, 8, 5, 8
    X, y, g, _, _ = svi.make_cfg5(N, D, G)
    n_total, lr, seed, a0, b0 = 10.0 * N, 0.05, 5, 1.5, 0.8
    lj, latents = route_t._expression(D, G, n_total / N, a0, b0)
    data = {"X": X, "y": y, "Gm": np.eye(G, dtype=np.float32)[g]}
    eng = ReparamVI(lj, latents, data, n_samples=S, seed=seed, lr=lr, backend=DeviceBackend(ctx))
    assert eng.route.startswith("fused: bsc_glm_data_pass_groups"), (eng.route, eng.route_reason)
    hand = HierGLMReparamSVI(ctx.to_device(X), ctx.to_device(y), ctx.to_device(g), G, n_total=eng.plan.scale * N,
                             n_samples=S, seed=seed, lr=lr, a0=eng.plan.a0, b0=eng.plan.b0, ctx=ctx, lam0=eng.lam)
    for _ in range(3):
        eng.step()
        hand.step()
    g2 = g.astype(np.int32).copy()
    g2[::3] = -1
    a, b = _as_numpy(eng.predict(X, y, groups=g2)), _as_numpy(hand.predict(X, y, groups=g2))
    for k in NAMES:
        npt.assert_array_equal(a[k], b[k])
    with pytest.raises(NotImplementedError, match="per-draw, per-group term"):
        eng.predict(X, y)
