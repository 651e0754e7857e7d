"""The float64 reference of the Student-t route (tests/_glm_studentt_ref.py) checked against scipy and itself, what a
float32 pass can reach against the device bounds, and the driver's host side; no device needed.

Most of this file checks the REFERENCE and the bounds, not the product: it is what licenses EPS and the GPU tests'
yardstick.  Every test imports tests/_glm_studentt_ref.py, which is new with the feature; the tests of the driver and of
svi/predict.py's tables are the ones that test the product here.

 * log p against scipy.stats.t.logpdf(y, nu, loc = l, scale = sigma) at every nu of the list, and against
   scipy.stats.cauchy.logpdf at nu = 1, rtol 1e-10 with an absolute 1e-9 (the outliers' densities are -20 .. -40);
 * G and T against central differences of the reference's own ell in w and tau; the tolerance is the difference between
   the quotients at h and h / 2 (three times the finer one's truncation error);
 * at nu = 1e6 and |z| <= 2, ell, G and T are the Gaussian's within the reference's own tolerance, EPS times the bound
   quantities (the two densities differ by z^4 / (4 nu) - z^2 / (2 nu) + O(1 / nu) per row, 4e-6 at most here);
 * the residual is bounded by k (nu + 1) / (2 sqrt nu), reached at z^2 = nu, whatever the outlier;
 * a zero-weight row holding NaN, +-inf or 0 changes nothing;
 * the device's link replayed in plain float32 (link_f32, data_pass_f32) within 1e-6 of the bound quantities at every
   shape tests/test_glm_studentt_gpu.py runs and every nu, |z| from 1e-3 to 1e4 and beyond; log1p keeps its digits at
   nu = 1e6;
 * EPS times the bound is below 1e-3 of the results where the data have the size of the noise (test docstring);
 * the constructor's refusals, each before a device is asked for, and the family tables."""
import math

import numpy as np
import numpy.testing as npt
import pytest
from scipy import stats

import _glm_obs_ref as obs
import _glm_studentt_ref as ref

F32_REACH = 1e-6        # what a plain float32 evaluation is held to, of the bound quantities (the device: ref.EPS = 2e-5)


def test_the_list_of_nu_and_eps_are_the_ones_the_issue_names():
    import _glm_lognormal_ref as lognormal
    assert ref.EPS is lognormal.EPS and ref.EPS == 2e-5
    assert ref.NUS == (1.0, 2.5, 4.0, 30.0, 1.0e6)
    assert all(float(np.float32(nu)) == nu for nu in ref.NUS)
    assert (ref.TAU_LO, ref.TAU_HI, ref.Z_LO, ref.Z_HI) == (-3.0, 5.0, 1e-3, 1e4)


@pytest.mark.parametrize("nu", ref.NUS)
def test_row_logpdf_is_scipys_student_t_density(nu):
    X, y, W, lis, o, _ = ref.make_inputs(200, 8, 6, 2, mode="offset")
    L = obs.logits(X, W, o)
    sigma = np.exp(-lis.astype(np.float64))[None, :]
    y64 = y.astype(np.float64)[:, None]
    got = ref.row_logpdf(L, y, lis, nu)
    npt.assert_allclose(got, stats.t.logpdf(y64, nu, loc=L, scale=sigma), rtol=1e-10, atol=1e-9)
    if nu == 1.0:
        npt.assert_allclose(got, stats.cauchy.logpdf(y64, loc=L, scale=sigma), rtol=1e-10, atol=1e-9)
    z = np.abs((y64 - L) / sigma)
    assert z[:, 0].min() < 2e-3 and z[:, 0].max() > 5e3 and lis.min() == ref.TAU_LO and lis.max() == ref.TAU_HI
    # and ell is its sum: nothing is left out
    ell, _, _ = ref.data_pass(X, y, W, lis, nu, o, None)
    npt.assert_allclose(ell, got.sum(axis=0), rtol=1e-12)


@pytest.mark.parametrize("nu", ref.NUS)
def test_G_and_T_are_the_derivatives_of_ell(nu):
    B, D, S = 60, 4, 3
    rs = np.random.RandomState(1)
    X, _, W, lis, o, v = ref.make_inputs(B, D, S, 1, tau=[-1.0, 0.25, 1.25])
    q = lambda a: (np.round(a * 4096.0) / 4096.0).astype(np.float32)       # w +- h and tau +- h exact in float32
    W, lis = q(W), q(lis)
    # |z| up to 30 at the first draw: a central difference over an outlier at 1e4 would need a step far below 2^-8
    y = (obs.logits(X, W, o)[:, 0] + rs.choice([-1.0, 1.0], B) * np.exp(rs.uniform(math.log(1e-3), math.log(30.0), B))
         / math.exp(float(lis[0]))).astype(np.float32)
    _, G, T = ref.data_pass(X, y, W, lis, nu, o, v)
    b_ell = ref.bounds(X, y, W, lis, nu, o, v)[0]

    def quotient(s, d, h):
        Wp, Wm, tp, tm = W.copy(), W.copy(), lis.copy(), lis.copy()
        if d is None:
            tp[s] += h
            tm[s] -= h
        else:
            Wp[s, d] += h
            Wm[s, d] -= h
        return (ref.data_pass(X, y, Wp, tp, nu, o, v)[0][s] - ref.data_pass(X, y, Wm, tm, nu, o, v)[0][s]) / (2 * h)

    h = 2.0 ** -10
    for s in range(S):
        for d in list(range(D)) + [None]:
            coarse, fine = quotient(s, d, h), quotient(s, d, h / 2)
            tol = abs(coarse - fine) + 1e-12 * b_ell[s] / h          # truncation, and the rounding of ell over 2 h
            got = T[s] if d is None else G[s, d]
            assert abs(got - fine) <= tol, (s, d, got, fine, tol)
            assert tol <= 1e-3 * max(abs(got), 1.0)                  # the check is not vacuous
    assert np.abs(T).min() > 1e-2 and np.abs(G).max() > 1.0


def test_at_a_million_degrees_of_freedom_the_pass_is_the_gaussians():
    """nu = 1e6 and |z| <= 2 at every draw (one weight vector for all draws, the largest k at the first): log p differs
    from the Gaussian's by z^4 / (4 nu) - z^2 / (2 nu) + (c_nu + log(2 pi) / 2 = -1 / (4 nu)), at most 4e-6 - 2e-6 per
    row, and the tolerance per row is EPS (|tau| + |c_nu| + 1 + ...) >= 4e-5."""
    B, D, S, nu = 400, 8, 3, 1.0e6
    rs = np.random.RandomState(5)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = np.repeat((0.6 * rs.standard_normal((1, D))).astype(np.float32), S, axis=0)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    lis = np.array([0.5, -1.0, 0.0], np.float32)
    zeta = np.exp(rs.uniform(math.log(1e-3), math.log(2.0), B)) * rs.choice([-1.0, 1.0], B)
    y = (obs.logits(X, W, o)[:, 0] + 0.98 * zeta / math.exp(0.5)).astype(np.float32)
    z = np.exp(lis.astype(np.float64))[None, :] * (y.astype(np.float64)[:, None] - obs.logits(X, W, o))
    assert np.abs(z).max() <= 2.0 and np.abs(z).max() > 1.9
    got = ref.data_pass(X, y, W, lis, nu, o, v)
    want = ref.gaussian_pass(X, y, W, lis, o, v)
    bnd = ref.bounds(X, y, W, lis, nu, o, v)
    for g, w, b, name in zip(got, want, bnd, ("ell", "G", "T")):
        ratio = float((np.abs(g - w) / (ref.EPS * b)).max())
        print("nu = 1e6 against the Gaussian, %s: %.3g of the tolerance" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
    # (c_nu is a difference of two lnGamma values of 6.06e6: two float64 roundings of that size are 2.7e-9)
    assert abs(ref.log_norm(nu) + 0.5 * ref.nb.LOG_2PI + 0.25 / nu) < 3e-9
    # ... and at nu = 4 it is not: the check can fail
    far = ref.data_pass(X, y, W, lis, 4.0, o, v)
    assert (np.abs(far[0] - want[0]) > 100.0 * ref.EPS * bnd[0]).all()


@pytest.mark.parametrize("nu", ref.NUS)
def test_the_residual_is_bounded_whatever_the_outlier(nu):
    X, y, W, lis, o, v = ref.make_inputs(300, 8, 5, 6)
    r = ref._terms(X, y, W, lis, nu, o, v)[2]
    k = np.exp(lis.astype(np.float64))[None, :]
    cap = v.astype(np.float64)[:, None] * k * (nu + 1.0) / (2.0 * math.sqrt(nu))
    assert (np.abs(r) <= cap * (1.0 + 1e-12)).all() and np.abs(r).max() > 0
    z = k * (y.astype(np.float64)[:, None] - obs.logits(X, W, o))
    if nu <= 30.0:                                           # the gross outliers pull less than the rows at z^2 = nu
        far = (np.abs(z) > 1e3) & (v > 0)[:, None]
        assert far.any() and (np.abs(r)[far] <= 0.01 * cap[far] * max(nu, 1.0) ** 0.5 + 1e-300).all()


def test_zero_weight_rows_are_dropped_whatever_they_hold():
    X, y, W, lis, o, v = ref.make_inputs(40, 8, 4, 3)
    v[36:] = 0.0
    y[36:] = [0.0, np.nan, np.inf, -np.inf]
    o[36:] = [200.0, -1.0e30, 1.0e30, 0.0]
    keep = v > 0
    dead = y[~keep]
    assert np.isnan(dead).any() and (dead == np.inf).any() and (dead == -np.inf).any() and (dead == 0).any()
    for nu in ref.NUS:
        a = ref.data_pass(X, y, W, lis, nu, o, v)
        b = ref.data_pass(X[keep], y[keep], W, lis, nu, o[keep], v[keep])
        a32 = ref.data_pass_f32(X, y, W, lis, nu, o, v)
        for p, q, p32 in zip(a, b, a32):
            assert np.isfinite(p).all() and np.isfinite(p32).all()
            npt.assert_allclose(p, q, rtol=1e-13, atol=1e-13 * np.abs(q).max())


@pytest.mark.parametrize("nu", ref.NUS)
def test_predictive_reference_against_scipy(nu):
    B, D, S = 120, 8, 16
    X, y, W, lis, o, _ = ref.make_inputs(B, D, S, 4, mode="offset")
    out = ref.predict(X, W, lis, nu, y, o)
    L = obs.logits(X, W, o)
    sigma = np.exp(-lis.astype(np.float64))[None, :]
    npt.assert_allclose(out["mean"], L.mean(axis=1), rtol=1e-12)
    if nu > 2.0:
        v = np.broadcast_to(stats.t.var(nu, scale=sigma), L.shape)
        npt.assert_allclose(out["var"], v.mean(axis=1) + L.var(axis=1), rtol=1e-10)       # law of total variance
        npt.assert_allclose(stats.t.mean(nu, loc=L, scale=sigma), L, rtol=1e-12)          # the location is the mean
    else:
        assert np.isposinf(out["var"]).all() and not np.isfinite(stats.t.var(nu))      # (scipy: NaN at nu <= 1)
    npt.assert_allclose(stats.t.median(nu, loc=L, scale=sigma), L, rtol=1e-12, atol=1e-12)    # and always the median
    lp = stats.t.logpdf(y.astype(np.float64)[:, None], nu, loc=L, scale=sigma)
    mx = lp.max(axis=1, keepdims=True)
    npt.assert_allclose(out["lpd"], mx[:, 0] + np.log(np.exp(lp - mx).mean(axis=1)), rtol=1e-9, atol=1e-9)
    npt.assert_allclose(out["lpd_sum"], out["lpd"].sum(), rtol=1e-12)
    b = ref.predict_bounds(X, W, lis, nu, y, o)
    assert all((b[q] > 0).all() for q in ("mean", "lpd")) and b["lpd_sum"] > 0 and np.isfinite(b["var"]).all()
    assert (b["var"] > 0).all()


# ---- what float32 reaches ---------------------------------------------------------------------------------------------

def test_the_quotient_form_of_log1p_keeps_its_digits_at_a_million_degrees_of_freedom():
    """r = z^2 / nu = 1e-6 z^2 and ((nu + 1) / 2) log1p(r) = z^2 / 2: log(1 + r) alone loses the digits of r that 1 + r
    rounds away (up to 6e-8 / r of the result, 6 % at r = 1e-6), the quotient form log(t) r / (t - 1) gives them back.
    The replay's term of ell against float64, z from 1e-3 to 1e4, relative to the term's own size."""
    nu = 1.0e6
    z = np.exp(np.linspace(math.log(1e-3), math.log(1e4), 4001))
    y = np.concatenate([z, -z]).astype(np.float32)
    l = np.zeros((y.shape[0], 1), np.float32)
    tau = np.zeros(1, np.float32)
    t_ell, res, t_T = ref.link_f32(l, y, np.ones_like(y), tau, nu)
    z64 = y.astype(np.float64)
    want = ref.log_norm(nu) - 0.5 * (nu + 1.0) * np.log1p(z64 * z64 / nu)
    size = abs(ref.log_norm(nu)) + 0.5 * (nu + 1.0) * np.log1p(z64 * z64 / nu)
    err = np.abs(t_ell[:, 0] - want) / size
    print("log1p at nu = 1e6: worst error %.3g of the term's size" % err.max())
    assert err.max() <= 4.0 * float(np.finfo(np.float32).eps)
    naive = ref.log_norm(nu) - 0.5 * (nu + 1.0) * np.log((np.float32(1.0) + (y * y) * np.float32(1e-6)).astype(np.float64))
    assert (np.abs(naive - want) / size).max() > 1e-3           # the plain form does lose them
    npt.assert_allclose(res[:, 0], (nu + 1.0) * z64 / (nu + z64 * z64), rtol=4e-7)
    assert (np.abs(t_T[:, 0] - nu * (1.0 - z64 * z64) / (nu + z64 * z64)) <= 4e-7 * (1.0 + z64 * z64)).all()


def _f32_ratios(X, y, W, lis, nu, o, v):
    got = ref.data_pass_f32(X, y, W, lis, nu, o, v)
    want = ref.data_pass(X, y, W, lis, nu, o, v)
    bnd = ref.bounds(X, y, W, lis, nu, o, v)
    assert all(np.isfinite(g).all() for g in got)
    return [float((np.abs(g - w) / b).max()) for g, w, b in zip(got, want, bnd)]


MI355X_CUS = 256      # tests/test_glm_studentt_gpu.py sizes two batches from the device's CU count

GPU_SHAPES = [(1003, 12, 8), (517, 200, 11), (1003, 256, 3), (1029, 256, 8), (1029, 256, 11),
              (MI355X_CUS * 4 * 16 * 2 + 5, 256, 8), (MI355X_CUS * 4 * 8 * 2 + 3, 12, 8)]


@pytest.mark.parametrize("B,D,S", GPU_SHAPES)
def test_plain_float32_stays_inside_the_bounds_over_the_whole_grid(B, D, S):
    """Every nu of the list at every shape of the GPU tests: tau over [-3, 5], |z| from 1e-3 to 1e4 at the first draw and
    up to e^8 times that at the others, the dead rows holding NaN, +-inf and 0."""
    X, y, W, lis, o, v = ref.make_inputs(B, D, S, seed=B * 7 + D + S)
    assert ref.TAU_LO == lis.min() and lis.max() == ref.TAU_HI
    z0 = np.abs(math.exp(float(lis[0])) * (y.astype(np.float64) - obs.logits(X, W, o)[:, 0]))[v > 0]
    assert z0.min() < 2e-3 and z0.max() > 5e3
    nus = ref.NUS if B < 10000 else (1.0, 1.0e6)            # (the two large batches: the two ends)
    for nu in nus:
        r_ell, r_G, r_T = _f32_ratios(X, y, W, lis, nu, o, v)
        print("B=%d D=%d S=%d nu=%g: error / bound quantity ell %.3g, G %.3g, T %.3g" % (B, D, S, nu, r_ell, r_G, r_T))
        assert max(r_ell, r_G, r_T) <= F32_REACH


@pytest.mark.parametrize("tau", [ref.TAU_LO, 1.0, ref.TAU_HI])
@pytest.mark.parametrize("nu", ref.NUS)
def test_the_tolerance_is_a_thousandth_of_the_results_where_the_data_have_the_size_of_the_noise(tau, nu):
    """EPS times the bound quantity against the float64 results themselves, for the reference alone.  The bound counts the
    conditioning of z = k (y - l) on the rounding of y and l, k (|y| + a) eps: where the data are hundreds of sigma
    away from 0 (tau = 5 with logits of size 1) that term is the whole bound and no float32 pass can do better, so the
    grid for THIS statement has the data at the size of the noise (unit = 1 / k) and ONE draw, the one the responses
    are laid out for: |z| log-uniform over [1e-3, 1e4], as designed.  Entries that
    are sums of both signs pass through 0 -- T does at the scale the fit is looking for, every column of G but the
    intercept's does by the symmetry of X -- so the statement is made for ell and T per draw and for the intercept
    column of G, where 70 % of the rows pull the same way, at B = 4003, large enough that the sums' means stand clear
    of their fluctuation (T per row at nu = 1 is -0.14 for a log-uniform |z| over [1e-3, 1e4], its standard deviation
    over 3200 kept rows 0.03)."""
    X, y, W, lis, o, v = ref.make_inputs(4003, 12, 1, seed=11, tau=tau, unit=math.exp(-tau))
    ell, G, T = ref.data_pass(X, y, W, lis, nu, o, v)
    b_ell, b_G, b_T = ref.bounds(X, y, W, lis, nu, o, v)
    r = (float((ref.EPS * b_ell / np.abs(ell)).max()), float((ref.EPS * b_G[:, 0] / np.abs(G[:, 0])).max()),
         float((ref.EPS * b_T / np.abs(T)).max()))
    print("tau=%g nu=%g: EPS * bound / |result|  ell %.3g, G[:, 0] %.3g, T %.3g" % ((tau, nu) + r))
    assert max(r) <= 1e-3, r


# ---- the driver's host side ---------------------------------------------------------------------------------------------

def test_constructor_refusals_need_no_device():
    from bayesic_amd.svi import StudentTReparamSVI
    X = np.zeros((5, 4), np.float32)
    y = np.arange(-2, 3, dtype=np.float32)
    for wrong in (0.0, -1.0, np.nan, np.inf, -np.inf, 1e39, "four", None):
        with pytest.raises(ValueError, match="df=.* must be a finite number > 0"):
            StudentTReparamSVI(X, y, df=wrong)
    for wrong in (np.nan, np.inf, -np.inf, 1e39):
        bad = y.astype(np.float64)
        bad[2] = wrong
        with pytest.raises(ValueError, match="y must be finite"):
            StudentTReparamSVI(X, bad)
    with pytest.raises(ValueError, match=r"lam0 has 8 entries; \[m \| rho\] over \[w \(4\) \| tau\] needs 10"):
        StudentTReparamSVI(X, y, lam0=np.zeros(8))
    with pytest.raises(ValueError, match="covariance"):
        StudentTReparamSVI(X, y, covariance="nope")
    with pytest.raises(ValueError, match="a0 and b0"):
        StudentTReparamSVI(X, y, a0=0.0)
    with pytest.raises(ValueError, match=r"n_samples must be in \[1, 64\]"):
        StudentTReparamSVI(X, y, n_samples=65)
    with pytest.raises(TypeError):
        StudentTReparamSVI(X, y, exposure=np.ones(5, np.float32))        # there is no exposure keyword
    with pytest.raises(TypeError):
        StudentTReparamSVI(X, y, upper=np.full(5, np.inf, np.float32))   # and no upper ends


def test_set_batch_checks_y_and_params_report_both_means_and_df():
    import torch
    from bayesic_amd.svi.glm_studentt import StudentTReparamSVI, check_df
    assert check_df(4) == 4.0 and check_df(np.float32(2.5)) == 2.5
    m = StudentTReparamSVI.__new__(StudentTReparamSVI)
    m.D, m.ctx, m.df = 4, None, 2.5
    X = torch.zeros((5, 4))
    y = torch.tensor([0.5, -2.0, 0.0, 4.0e30, -1.0e-3])
    m.set_batch(X, y)
    assert m._yarg is m.y and m.B == 5 and m.offset is None and m.weights is None
    npt.assert_array_equal(m.y.numpy(), y.numpy())                           # any finite float, as it is
    with pytest.raises(ValueError, match="y must be finite"):
        m.set_batch(X, torch.tensor([0.5, float("nan"), 0.0, 1.0, 2.0]))
    with pytest.raises(ValueError, match="y must be finite"):
        m.set_batch(X, torch.tensor([0.5, float("-inf"), 0.0, 1.0, 2.0]))
    with pytest.raises(TypeError):
        m.set_batch(X, y, upper=torch.ones(5))
    with pytest.raises(TypeError):
        m.set_batch(X, y, exposure=torch.ones(5))
    m.set_batch(1234, 5678, rows=5)                                          # raw pointers are taken as they are
    assert m._yarg == 5678 and m.y is None
    with pytest.raises(TypeError):
        m.predict(X, y, exposure=torch.ones(5))
    with pytest.raises(TypeError):
        m.heldout_lpd(X, y, upper=torch.ones(5))
    # params(): E_q[e^tau], E_q[e^{-tau}] and df, mean-field and full (the marginal variance of tau: the last row of L)
    D = 4
    m.covariance_kind = "diag"
    lam = np.concatenate([[0.1, 0.2, 0.3, 0.4, 0.7], np.log([0.1, 0.1, 0.1, 0.1, 0.3])])
    m._lam, m.t = torch.from_numpy(lam)[None, :], 0
    p = m.params()
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(0.7 + 0.045), rtol=1e-12)
    npt.assert_allclose(p["sigma_mean"], math.exp(-0.7 + 0.045), rtol=1e-12)
    assert p["df"] == 2.5
    from bayesic_amd.svi._reparam_base import unpack_full
    m.covariance_kind = "full"
    P = D + 1
    rs = np.random.RandomState(0)
    lam_full = np.concatenate([lam[:P], 0.1 * rs.standard_normal(P * (P + 1) // 2)])
    m._lam = torch.from_numpy(lam_full)[None, :]
    L = unpack_full(lam_full, P)[1]
    var = float((L[D] ** 2).sum())
    p = m.params()
    npt.assert_allclose(p["inv_sigma_mean"], math.exp(0.7 + 0.5 * var), rtol=1e-12)
    npt.assert_allclose(p["sigma_mean"], math.exp(-0.7 + 0.5 * var), rtol=1e-12)
    assert p["df"] == 2.5


def test_data_pass_hands_df_to_the_entry_point_behind_S():
    from bayesic_amd import _ffi
    from bayesic_amd.svi.glm_studentt import StudentTReparamSVI
    from ctypes import c_double, c_int32

    class Ctx:
        def call(self, name, *args):
            self.seen = (name, args)

    m = StudentTReparamSVI.__new__(StudentTReparamSVI)
    m.ctx, m.df, m.B, m.D, m.S, m.t = Ctx(), 30.0, 7, 4, 8, 0
    m._Xarg, m._ldx, m._yarg, m._oarg, m._varg = 11, 4, 12, None, 13
    m._W, m._loginvscale, m.ell, m.G, m.T = [14, 0], [15, 16], 17, 18, 19
    m.data_pass()
    name, args = m.ctx.seen
    assert name == "bsc_glm_studentt_data_pass"
    assert args == (11, 4, 12, None, 13, 7, 4, 14, 15, 8, 30.0, 17, 18, 19)
    # the bound signatures: the lognormal pass's with one double behind S (the context is argument 0)
    for ours, twin in (("bsc_glm_studentt_data_pass", "bsc_glm_lognormal_data_pass"),
                       ("bsc_studentt_predict_pass", "bsc_lognormal_predict_pass")):
        a, b = _ffi.SIGNATURES[ours][1], _ffi.SIGNATURES[twin][1]
        at = len(a) - 1 - a[::-1].index(c_int32)
        assert a[at + 1] is c_double and a[:at + 1] + a[at + 2:] == b and len(a) == len(b) + 1
    assert _ffi.SIGNATURES["bsc_glm_studentt_update"] == _ffi.SIGNATURES["bsc_glm_lognormal_update"]


def test_family_of_and_the_family_lists_take_the_new_entry_and_keep_the_old():
    from bayesic_amd.svi import predict as mod
    from bayesic_amd.svi import LogNormalReparamSVI, StudentTReparamSVI
    import bayesic_amd.svi as svi
    assert "StudentTReparamSVI" in svi.__all__
    assert mod.family_of(StudentTReparamSVI.__new__(StudentTReparamSVI)) == "studentt"
    assert mod.family_of(LogNormalReparamSVI.__new__(LogNormalReparamSVI)) == "lognormal"
    assert mod.FAMILY_TABLE["studentt"] == mod.Family("bsc_studentt_predict_pass", "location", True, None)
    assert mod.SCALAR_PASSES == {"negbin": "bsc_nb_predict_pass", "gamma": "bsc_gamma_predict_pass",
                                 "weibull": "bsc_weibull_predict_pass"}
    assert mod.LOGIT_SCALAR_PASSES == {"beta": "bsc_beta_predict_pass"}
    assert mod.SCALAR_FAMILIES == {"negbin": 0, "gamma": 1, "weibull": 2}
    assert mod.FAMILIES == {"gaussian": 0, "logistic": 1, "poisson": 2}


def test_predict_refuses_exposure_upper_and_groups_before_a_device_is_asked_for():
    from bayesic_amd.svi import StudentTReparamSVI
    from bayesic_amd.svi import predict as mod
    m = StudentTReparamSVI.__new__(StudentTReparamSVI)
    m.D, m.ctx, m.df = 4, None, 4.0
    X = np.zeros((5, 4), np.float32)
    y = np.ones(5, np.float32)
    with pytest.raises(ValueError, match="upper= .* belongs to the Weibull model, not studentt"):
        mod.predict(m, X, y, upper=np.ones(5, np.float32))
    with pytest.raises(ValueError, match="groups= belongs to the random-intercept model"):
        mod.predict(m, X, y, groups=np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="exposure belongs to the Poisson rate model; the studentt model takes offset="):
        mod.predict(m, X, y, exposure=np.ones(5, np.float32))
