"""The posterior predictive of the mixture on the device: bsc_mog_predictive_params and bsc_mog_predict_pass
(csrc/bsc_mog_predict.hip) against the float64 restatement of tests/_mog_predict_ref.py, and MoGNatGradSVI.predict /
heldout_lpd / predictive_params on top of them.

Tolerances (eps = 2e-5 of the bound quantity B_nk = |c_k| + sum_d h_kd log1p(u_nkd), what the project's device tests use;
the reference takes the float32 table and float32 rows and computes in float64):
 * table: every entry within 2 float32 ulps of the rounded float64 value;
 * lpd:   |lpd - lpd64| <= eps sum_k R64_nk B_nk, the first-order image of an eps B error on each logit;
 * R:     the same error to first order, dR_k = R_k (dl_k - sum_j R_j dl_j), plus what float32 cannot hold:
          |R - R64| <= R64 (eps (B_nk + sum_j R64_nj B_nj) + 2^-23) + 2^-126; every row sums to 1 within 1e-5;
 * label: equal to the float64 argmax on every row whose two largest float64 logits are at least 4e-5 max_k B_nk apart;
          at most 1 % of a case's rows may be nearer than that (tests/test_mog_predict_cpu.py holds the shares);
 * lpd_sum: the float64 sum of the device's own lpd at rtol 1e-6, and the same bits from two runs.

MEASURED ON AN MI355X (256 CUs; every case prints its own figures: -s), worst error over its bound:
 * table: equal to the rounded float64 table in every entry (0.0 ulps) at K = 37, D = 9 and K = 64, D = 16, a = 1e5 included;
 * lpd: 1.3e-3 (N = 1) to 7.3e-3 (N = 20 000, D = 12, K = 40) over the parity cases, 6.4e-3 at a = 1e5 and centres near 170,
   8.2e-3 to 9.5e-3 at two and three trips per wave, 5.1e-3 to 5.8e-3 through the driver;
 * R: 8.0e-3 to 1.5e-2 over the entries of at least 1e-30; over ALL entries 0.80 to 0.997 wherever a row has an entry below
   the smallest normal float32 -- v_exp_f32 returns 0 there, the error is the entry itself, and the bound's 2^-126 term is
   there for exactly that (the ratio tends to 1 from below as such an entry tends to 2^-126; it cannot pass it);
   |sum_k R - 1| 7.6e-7 at most;
 * label: no wrong label off the near-ties in any case; near-ties 0 to 0.13 % of a case's rows (cap 1 %); every label right
   on the exact data at 1, 2 and 3 trips per wave (4 101, 262 213 and 524 357 rows);
 * every allowed choice of outputs, ldr = K + 3 and two runs give the same bits; sentinels untouched everywhere;
 * held-out lpd per row -8.718540 (K = 5), -13.621817 (K = 2), -15.446924 (K = 1): the float64 figures to seven digits.
"""
import itertools

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _mixture_ref as mr
import _mog_predict_ref as pr
from oracle import svi
from test_regression_multi_tile_gpu import _guard_untouched, _guarded   # 64 sentinel elements past the end

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cu(ctx):
    return int(ctx.info()["cu_count"])


def _params(ctx, eta, K, D):
    Pt, c = ctx.empty((K, 3 * D)), ctx.empty(K)
    ctx.call("bsc_mog_predictive_params", ctx.to_device(np.asarray(eta), torch.float64), K, D, Pt, c)
    return Pt, c


def _device_rows(ctx, X, ldx=None, offset=0):
    """X on the device as the pass is to read it: rows ldx apart (NaN between them), `offset` floats into its buffer."""
    N, D = X.shape
    ldx = ldx or D
    wide = np.full(offset + N * ldx, np.nan, np.float32)
    wide[offset:].reshape(N, ldx)[:, :D] = X
    return ctx.to_device(wide)[offset:].view(N, ldx)[:, :D], ldx


def _pass(ctx, Xd, ldx, K, Ptd, cd, outputs=("lpd", "label", "R", "sum"), ldr=None):
    """-> dict of host arrays of the outputs asked for; lpd, label and R carry 64 sentinels past N whose bits are checked."""
    N, D = Xd.shape
    ldr = ldr or K
    buf = dict(lpd=_guarded(ctx, N) if "lpd" in outputs else None,
               label=_guarded(ctx, N) if "label" in outputs else None,       # (int32 results in a float32 buffer)
               R=_guarded(ctx, N * ldr) if "R" in outputs else None,
               sum=ctx.empty(1, torch.float64) if "sum" in outputs else None)
    ctx.call("bsc_mog_predict_pass", Xd, ldx, N, D, K, Ptd, cd, buf["lpd"], buf["label"], buf["R"], ldr, buf["sum"])
    ctx.sync()
    out = {}
    if "lpd" in outputs:
        _guard_untouched(buf["lpd"], N)
        out["lpd"] = buf["lpd"][:N].cpu().numpy()
    if "label" in outputs:
        _guard_untouched(buf["label"], N)
        out["label"] = buf["label"][:N].view(torch.int32).cpu().numpy()
    if "R" in outputs:
        _guard_untouched(buf["R"], N * ldr)
        full = buf["R"][:N * ldr].view(N, ldr).cpu().numpy()
        if ldr > K:       # the columns between the rows belong to the caller
            npt.assert_array_equal(full[:, K:].view(np.int32), np.full((N, ldr - K), -777.0, np.float32).view(np.int32))
        out["R"] = full[:, :K]
    if "sum" in outputs:
        out["sum"] = buf["sum"].cpu().numpy()
    return out


def _assert_outputs(got, ref, tag):
    """The module docstring's tolerances; prints the worst error over its bound."""
    N = ref["lpd"].shape[0]
    if N == 0:
        assert got["lpd"].size == 0 and got["label"].size == 0 and got["R"].size == 0
        assert got["sum"][0] == 0.0
        print("%s: no rows, lpd_sum = 0" % tag)
        return
    assert np.isfinite(got["lpd"]).all() and np.isfinite(got["R"]).all()
    r_lpd = float((np.abs(got["lpd"] - ref["lpd"]) / pr.lpd_bound(ref)).max())
    ratio_R = np.abs(got["R"] - ref["R"]) / pr.resp_bound(ref)
    r_R = float(ratio_R.max())
    r_R_normal = float(ratio_R[ref["R"] >= 1e-30].max())      # (printed only: see the module docstring)
    rows1 = float(np.abs(got["R"].astype(np.float64).sum(axis=1) - 1.0).max())
    keep = ~ref["tie"]
    wrong = int((got["label"][keep] != ref["label"][keep]).sum())
    print("%s: lpd %.3g, R %.3g (entries >= 1e-30: %.3g) of their bounds; |sum_k R - 1| %.2g; %d of %d rows near-ties; "
          "%d labels wrong" % (tag, r_lpd, r_R, r_R_normal, rows1, int(ref["tie"].sum()), N, wrong))
    assert r_lpd <= 1.0
    assert r_R <= 1.0
    assert rows1 <= 1e-5
    assert ref["tie"].mean() <= pr.TIE_CAP
    assert wrong == 0
    assert ((got["label"] >= 0) & (got["label"] < ref["R"].shape[1])).all()
    npt.assert_allclose(got["sum"][0], got["lpd"].astype(np.float64).sum(), rtol=1e-6)


# ---- 1. the table -----------------------------------------------------------------------------------------------------

def _perturbed_eta(K, D):
    rs = np.random.RandomState(100 * K + D)
    X = rs.standard_normal((4 * K, D)) * 3
    alpha, m, kappa, a, b = svi.mog_unpack(svi.mog_init_eta(X, K, D, seed=3), K, D)
    alpha = alpha * rs.uniform(1, 5, K)
    m = m + 0.3 * rs.standard_normal((K, D))
    kappa, a, b = kappa * rs.uniform(1, 50, (K, D)), a * rs.uniform(1, 20, (K, D)), b * rs.uniform(0.5, 5, (K, D))
    a[::5, ::3], b[::5, ::3], kappa[::5, ::3] = 1.0e5, 0.9e5, 2.0e5      # lnGamma(a + 1/2) - lnGamma(a) cancels here
    m[::5, ::3] += 170.0
    return pr.pack(alpha, m, kappa, a, b)


@pytest.mark.parametrize("K, D", [(37, 9), (64, 16)])
def test_table_is_the_rounded_float64_table(ctx, K, D):
    eta = _perturbed_eta(K, D)
    Pt, c = _params(ctx, eta, K, D)
    ctx.sync()
    want_P, want_c = pr.table_f32(eta, K, D)
    worst = 0.0
    for got, want in ((Pt.cpu().numpy(), want_P), (c.cpu().numpy(), want_c)):
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert (ulps <= 2.0).all()
    print("K=%d D=%d: table within %.1f ulps" % (K, D, worst))


# ---- 2. parity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N, D, K", pr.PARITY_SHAPES)
def test_pass_matches_float64(ctx, N, D, K):
    X, eta, Pt, c, ref = pr.parity_reference(N, D, K)
    Xd, ldx = _device_rows(ctx, X)
    got = _pass(ctx, Xd, ldx, K, ctx.to_device(Pt), ctx.to_device(c))
    _assert_outputs(got, ref, "N=%d D=%d K=%d" % (N, D, K))
    again = _pass(ctx, Xd, ldx, K, ctx.to_device(Pt), ctx.to_device(c))
    for name in got:                                                     # two runs, the same bits
        npt.assert_array_equal(got[name].view(np.int32 if got[name].dtype.itemsize == 4 else np.int64),
                               again[name].view(np.int32 if again[name].dtype.itemsize == 4 else np.int64))


def test_device_table_and_pass_together(ctx):
    """The pass on the device's own table, as the driver runs it."""
    X, eta, _, _, _ = pr.parity_reference(1003, 16, 64)
    Ptd, cd = _params(ctx, eta, 64, 16)
    ref = pr.predict(X, Ptd.cpu().numpy(), cd.cpu().numpy())
    Xd, ldx = _device_rows(ctx, X)
    _assert_outputs(_pass(ctx, Xd, ldx, 64, Ptd, cd), ref, "device table")


# ---- 3. precision -----------------------------------------------------------------------------------------------------

def test_well_fitted_components_far_from_the_origin(ctx):
    """a = 1e5, kappa = 2e5, centres near 170: the plain float32 log(1 + u) would miss the tolerance 112-fold
    (tests/test_mog_predict_cpu.py)."""
    X, eta = pr.precision_case()
    Pt, c = pr.table_f32(eta, 8, 16)
    Xd, ldx = _device_rows(ctx, X)
    _assert_outputs(_pass(ctx, Xd, ldx, 8, ctx.to_device(Pt), ctx.to_device(c)), pr.predict(X, Pt, c), "a=1e5")


# ---- 4. exact accounting, 5. several tiles per wave ------------------------------------------------------------------

def _rows(n_iter, cu):
    N = pr.rows_for(n_iter, cu)
    g = pr.grid(N, cu)
    assert g["n_iter"] == n_iter and N % pr.PT == 5, (N, cu, g)
    return N


@pytest.mark.parametrize("n_iter", [1, 2, 3])
def test_every_row_gets_its_own_label(ctx, cu, n_iter):
    """Well-separated integer data with labels pseudo-random in the row: a dropped, doubled or swapped tile shows."""
    N = 4101 if n_iter == 1 else _rows(n_iter, cu)
    K, D = 64, 16
    X, _, _, labels, _ = mr.estep_exact_data(N, K, D)
    Pt, c = pr.table_f32(pr.exact_eta(K, D), K, D)
    Xd, ldx = _device_rows(ctx, X)
    got = _pass(ctx, Xd, ldx, K, ctx.to_device(Pt), ctx.to_device(c), outputs=("lpd", "label", "sum"))
    npt.assert_array_equal(got["label"], labels)
    npt.assert_allclose(got["sum"][0], got["lpd"].astype(np.float64).sum(), rtol=1e-6)


@pytest.mark.parametrize("D, ldx", [(16, 16), (12, 13)])
@pytest.mark.parametrize("n_iter", [1, 2, 3])
def test_several_tiles_per_wave(ctx, cu, n_iter, D, ldx):
    """The ragged last tile after n_iter - 1 full sweeps; at D = 12 the rows are 13 floats apart with NaN between them."""
    K = 5
    N = _rows(n_iter, cu)
    X, eta = pr.fitted_case(N, D, K)
    Pt, c = pr.table_f32(eta, K, D)
    Xd, ldx = _device_rows(ctx, X, ldx)
    got = _pass(ctx, Xd, ldx, K, ctx.to_device(Pt), ctx.to_device(c))
    _assert_outputs(got, pr.predict(X, Pt, c), "n_iter=%d D=%d ldx=%d N=%d" % (n_iter, D, ldx, N))


# ---- 6. views, optional outputs, refusals ------------------------------------------------------------------------------

def _bits(a):
    return a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)


@pytest.mark.parametrize("N, D, K", [(1003, 16, 64), (4097, 5, 64)])
def test_every_allowed_choice_of_outputs_gives_the_same_bits(ctx, N, D, K):
    X, eta, Pt, c, ref = pr.parity_reference(N, D, K)
    Xd, ldx = _device_rows(ctx, X, offset=1)                 # 4-byte, not 16-byte aligned
    assert Xd.data_ptr() % 16 == 4
    Ptd, cd = ctx.to_device(Pt), ctx.to_device(c)
    full = _pass(ctx, Xd, ldx, K, Ptd, cd)
    _assert_outputs(full, ref, "misaligned N=%d D=%d" % (N, D))
    names = ("lpd", "label", "R", "sum")
    for n in (1, 2, 3):
        for chosen in itertools.combinations(names, n):
            got = _pass(ctx, Xd, ldx, K, Ptd, cd, outputs=chosen)
            for name in chosen:
                npt.assert_array_equal(_bits(got[name]), _bits(full[name]), err_msg="%s of %s" % (name, chosen))
    wide = _pass(ctx, Xd, ldx, K, Ptd, cd, ldr=K + 3)        # rows of R 67 floats apart
    for name in names:
        npt.assert_array_equal(_bits(wide[name]), _bits(full[name]), err_msg="%s at ldr = K + 3" % name)


def test_refusals(ctx):
    from bayesic_amd._ffi import BayesicHipError
    X, P, c = ctx.zeros((8, 17)), ctx.zeros((65, 3 * 17)), ctx.zeros(65)
    lpd, s = ctx.zeros(8), ctx.zeros(1, torch.float64)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: no output"):
        ctx.call("bsc_mog_predict_pass", X, 17, 8, 16, 64, P, c, None, None, None, 64, None)
    with pytest.raises(BayesicHipError, match=r"status -3: bsc_mog_predict_pass: D=16 K=65 outside"):
        ctx.call("bsc_mog_predict_pass", X, 17, 8, 16, 65, P, c, lpd, None, None, 65, s)
    with pytest.raises(BayesicHipError, match=r"status -3: bsc_mog_predict_pass: D=17 K=64 outside"):
        ctx.call("bsc_mog_predict_pass", X, 17, 8, 17, 64, P, c, lpd, None, None, 64, s)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: bad ldx=15"):
        ctx.call("bsc_mog_predict_pass", X, 15, 8, 16, 64, P, c, lpd, None, None, 64, s)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: bad ldx=33554432"):
        ctx.call("bsc_mog_predict_pass", X, 1 << 25, 1, 16, 64, P, c, lpd, None, None, 64, s)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: bad ldr=63"):
        ctx.call("bsc_mog_predict_pass", X, 17, 8, 16, 64, P, c, None, None, ctx.zeros((8, 64)), 63, None)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: X must be 4-byte aligned"):
        ctx.call("bsc_mog_predict_pass", X.data_ptr() + 2, 17, 7, 16, 64, P, c, lpd, None, None, 64, s)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predict_pass: null pointer"):
        ctx.call("bsc_mog_predict_pass", None, 17, 8, 16, 64, P, c, lpd, None, None, 64, s)
    with pytest.raises(BayesicHipError, match=r"status -3: bsc_mog_predictive_params: K=1025"):
        ctx.call("bsc_mog_predictive_params", ctx.zeros(8, torch.float64), 1025, 1, P, c)
    with pytest.raises(BayesicHipError, match=r"status -1: bsc_mog_predictive_params: null pointer"):
        ctx.call("bsc_mog_predictive_params", None, 4, 1, P, c)


# ---- 7. the driver ------------------------------------------------------------------------------------------------------

def _by_hand(ctx, model, Xd, ldx):
    Ptd, cd = _params(ctx, model.eta.cpu().numpy(), model.K, model.D)
    return _pass(ctx, Xd, ldx, model.K, Ptd, cd)


@pytest.mark.parametrize("via", ["kernel", "executor"])
def test_driver_equals_the_entry_points_called_by_hand(ctx, via):
    from bayesic_amd.svi.mog import MoGNatGradSVI
    N, D, K = 5000, 16, 33
    X, _ = pr.fitted_case(N, D, K)
    eta0 = svi.mog_prior_eta(K, D)
    model = MoGNatGradSVI(X, K, eta0, svi.mog_init_eta(X, K, D, seed=4), ctx=ctx, via=via)
    for _ in range(2):
        model.step()
    held, ldx = _device_rows(ctx, X[:1234], ldx=19)          # a strided view: read in place
    out = model.predict(held, responsibilities=True)
    assert set(out) == {"lpd", "label", "lpd_sum", "resp"}
    assert out["lpd"].dtype == torch.float32 and out["label"].dtype == torch.int32
    assert out["lpd_sum"].dtype == torch.float64 and out["resp"].shape == (1234, K)
    want = _by_hand(ctx, model, held, ldx)
    for name, key in (("lpd", "lpd"), ("label", "label"), ("resp", "R"), ("lpd_sum", "sum")):
        npt.assert_array_equal(_bits(out[name].cpu().numpy()), _bits(want[key]), err_msg=name)
    assert set(model.predict(X[:1234])) == {"lpd", "label", "lpd_sum"}
    npt.assert_array_equal(_bits(model.predict(X[:1234])["lpd"].cpu().numpy()), _bits(want["lpd"]))      # a host array
    assert model.heldout_lpd(held) == want["sum"][0] / 1234
    Pt, c = model.predictive_params()
    _assert_outputs(want, pr.predict(X[:1234], Pt.cpu().numpy(), c.cpu().numpy()), "driver via=%s" % via)
    with pytest.raises(ValueError, match="15 columns"):
        model.predict(held[:, :15])


def test_driver_refuses_65_components_before_any_device_call(ctx):
    from bayesic_amd.svi.mog import MoGNatGradSVI
    K, D = 65, 4
    X = np.random.RandomState(0).standard_normal((300, D)).astype(np.float32)
    model = MoGNatGradSVI(X, K, svi.mog_prior_eta(K, D), svi.mog_init_eta(X, K, D), ctx=ctx)
    assert model.via == "executor"
    ctx.record_begin()
    try:
        for call in (lambda: model.predict(X), lambda: model.heldout_lpd(X)):
            with pytest.raises(NotImplementedError, match="K <= 64 components and D <= 16 columns"):
                call()
    finally:
        calls = ctx.record_end()
    assert calls == []


def test_heldout_lpd_orders_the_fits_as_float64_does(ctx):
    from bayesic_amd.svi.mog import MoGNatGradSVI
    train, held = pr.cluster_data()
    lpd = {}
    for K in (1, 2, 5):
        eta = pr.cluster_fit(K)
        model = MoGNatGradSVI(train, K, svi.mog_prior_eta(K, 5), eta, ctx=ctx)
        lpd[K] = model.heldout_lpd(held)
        ref = pr.predict(held, *pr.table_f32(eta, K, 5))
        assert abs(lpd[K] - ref["lpd"].mean()) <= pr.lpd_bound(ref).mean()
    print("held-out lpd per row on the device:", lpd)
    assert lpd[5] - lpd[2] >= 0.5 * pr.MARGIN_5_OVER_2
    assert lpd[5] - lpd[1] >= 0.5 * pr.MARGIN_5_OVER_1
