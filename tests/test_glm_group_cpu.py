"""The random-intercept GLM route on the CPU: the float64 reference (tests/_glm_group_ref.py) against finite
differences of its own ELBO integrand and against the one-hot identity with tests/_glm_obs_ref.py; a naive float32
evaluation against the bounds the device is held to (tests/test_glm_group_gpu.py); the host core of the group plan
through ctypes (no device); the driver's argument errors, raised before any device call; and a sanity run of the
reference stepper on a small synthetic hierarchy."""
import ctypes
import math

import numpy as np
import numpy.testing as npt
import pytest
import torch

import _glm_group_ref as ref
import _glm_obs_ref as obs

LINKS = ("logistic", "poisson")


def _inputs(link, B, D, J, S, seed):
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((B, D)) / math.sqrt(D)).astype(np.float32)
    W = (0.6 * rs.standard_normal((S, D))).astype(np.float32)
    Bm = (0.5 * rs.standard_normal((S, J))).astype(np.float32)
    g = rs.randint(J, size=B).astype(np.int32)
    o = rs.standard_normal(B).astype(np.float32)
    v = rs.uniform(0.0, 3.0, B).astype(np.float32)
    v[::5] = 0.0
    if link == "logistic":
        y = (rs.uniform(size=B) < 0.5).astype(np.float32)
    else:
        y = rs.poisson(1.5, size=B).astype(np.float32)
        peak = np.abs(ref.logits(X, g, W, Bm, o)).max()
        if peak > 3.5:
            W, Bm, o = ((a * (3.5 / peak)).astype(np.float32) for a in (W, Bm, o))
    return X, y, g, W, Bm, o, v


# ---- the reference --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("link", LINKS)
def test_reference_gradient_is_the_derivative_of_its_elbo(link):
    """Central differences of elbo_fixed_draws in every coordinate of lam (w, b, zeta; means and log deviations).  The
    reference's gradient is formed from float32-rounded draws, the integrand is float64 throughout: they agree to the
    float32 rounding of z (6e-8 relative) times the curvature, far inside rtol 1e-4 of the largest entry."""
    B, D, J, S = 80, 4, 3, 5
    X, y, g, _, _, o, v = _inputs(link, B, D, J, S, 1)
    P = D + J + 1
    rs = np.random.RandomState(2)
    lam = np.concatenate([0.3 * rs.standard_normal(P), math.log(0.2) + 0.1 * rs.standard_normal(P)])
    eps = ref.noise(D, J, S, 7, 0)
    scale, tau, a0, b0 = 3.0, 1.7, 1.5, 0.8
    W, Bm, zeta = ref.draw(lam, eps, D, J)
    ell, G, H = ref.data_pass(link, X, y, g, J, W, Bm, o, v)
    _, grad = ref.elbo_and_grad(lam, eps, W, Bm, zeta, ell, G, H, scale, tau, a0, b0)
    h = 1e-5
    fd = np.zeros_like(lam)
    for i in range(2 * P):
        e = np.zeros_like(lam)
        e[i] = h
        fd[i] = (ref.elbo_fixed_draws(link, lam + e, eps, X, y, g, J, scale, tau, a0, b0, o, v)
                 - ref.elbo_fixed_draws(link, lam - e, eps, X, y, g, J, scale, tau, a0, b0, o, v)) / (2 * h)
    assert np.abs(grad - fd).max() <= 1e-4 * np.abs(fd).max(), np.abs(grad - fd).max() / np.abs(fd).max()
    for lo, hi in ((0, D), (D, D + J), (P - 1, P)):           # w, b and zeta each carry a gradient worth checking
        assert np.abs(fd[lo:hi]).max() > 1e-2 and np.abs(fd[P + lo:P + hi]).max() > 1e-3


@pytest.mark.parametrize("link", LINKS)
def test_one_hot_identity_with_the_obs_reference(link):
    """With X' = [X | onehot(g)] and W' = [W | Bm], tests/_glm_obs_ref.data_pass gives the same ell, G in its first D
    columns and H^T in its last J."""
    B, D, J, S = 300, 8, 5, 4
    X, y, g, W, Bm, o, v = _inputs(link, B, D, J, S, 3)
    ell, G, H = ref.data_pass(link, X, y, g, J, W, Bm, o, v)
    X2 = np.concatenate([X, ref.onehot(g, J)], axis=1)
    W2 = np.concatenate([W, Bm], axis=1)
    ell2, G2 = obs.data_pass(link, X2, y, W2, o, v)
    npt.assert_allclose(ell, ell2, rtol=1e-13)
    npt.assert_allclose(G, G2[:, :D], rtol=1e-12, atol=1e-13)
    npt.assert_allclose(H, G2[:, D:], rtol=1e-12, atol=1e-13)
    npt.assert_allclose(ref.ell_bound(link, X, y, g, W, Bm, o, v), obs.ell_bound(link, X2, y, W2, o, v), rtol=1e-13)


def test_log_prior_is_the_oracles_at_unit_precision():
    from oracle import svi
    rs = np.random.RandomState(4)
    w, b, zeta = rs.standard_normal((3, 5)), rs.standard_normal((3, 4)), rs.standard_normal(3)
    z = np.concatenate([w, b, zeta[:, None]], axis=1)
    npt.assert_array_equal(ref.log_prior(w, b, zeta, 1.0, 1.3, 0.7), svi.bbvi_log_prior(z, 5, 4, 1.3, 0.7))
    # another tau_w is w's Gaussian alone
    want = svi.bbvi_log_prior(z, 5, 4) + (0.5 * 5 * math.log(2.0) - 0.5 * (w * w).sum(axis=1))
    npt.assert_allclose(ref.log_prior(w, b, zeta, 2.0), want, rtol=1e-14)


@pytest.mark.parametrize("B,D,J,S", [(37, 8, 3, 3), (2051, 256, 1000, 8), (4099, 64, 1, 5)])
@pytest.mark.parametrize("link", LINKS)
def test_a_naive_float32_evaluation_lies_inside_the_device_bounds(link, B, D, J, S):
    """Serial float32 sums, row after row: ell within 2e-5 of sum_n v_n (|y l| + A + 1), G within 1e-4 of max|G| and H
    within 1e-4 of max|H| -- the bounds tests/test_glm_group_gpu.py holds the device pass to."""
    X, y, g, W, Bm, o, v = _inputs(link, B, D, J, S, B + D)
    ell, G, H = ref.data_pass_f32(link, X, y, g, J, W, Bm, o, v)
    ell_r, G_r, H_r = ref.data_pass(link, X, y, g, J, W, Bm, o, v)
    bound = ref.ell_bound(link, X, y, g, W, Bm, o, v)
    e_ell = (np.abs(ell - ell_r) / bound).max()
    e_G = np.abs(G - G_r).max() / np.abs(G_r).max()
    e_H = np.abs(H - H_r).max() / np.abs(H_r).max()
    print("%s (%d, %d, %d, %d): ell err/bound %.3g, G err/max %.3g, H err/max %.3g" % (link, B, D, J, S, e_ell, e_G, e_H))
    assert e_ell <= 2e-5 and e_G <= 1e-4 and e_H <= 1e-4


def test_chunked_layout_round_trips():
    Bm = np.arange(11 * 3, dtype=np.float32).reshape(11, 3) + 1.0
    flat = ref.chunked(Bm)
    assert flat.shape == (2 * 3 * 8,)
    npt.assert_array_equal(ref.unchunk(flat, 11, 3), Bm)
    assert flat.reshape(2, 3, 8)[1, :, 3:].max() == 0.0          # the unused slots of the last chunk
    assert flat.reshape(2, 3, 8)[0, 2, 5] == Bm[5, 2]


# ---- the host core of the group plan, through ctypes ----------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from bayesic_amd import _ffi
    from bayesic_amd.build import build
    build()
    return _ffi.load_library()


HDR = 8


def _plan(lib, g, J):
    """(rc, perm, first segment of each group [J + 1], segments [(start, length, group)], n_segments)."""
    g = np.ascontiguousarray(g, np.int32)
    B = len(g)
    n = lib.bsc_glm_group_plan_size(B, J)
    assert n >= HDR + B + J + 1
    plan = np.full(n, -7, np.int32)
    n_seg = ctypes.c_int32(-1)
    rc = lib.bsc_glm_group_plan_host(g.ctypes.data if B else None, B, J, plan.ctypes.data, ctypes.byref(n_seg))
    if rc != 0:
        return rc, None, None, None, None
    ns = n_seg.value
    assert plan[1] == B and plan[2] == J and plan[3] == ns
    perm = plan[HDR:HDR + B]
    grp = plan[HDR + B:HDR + B + J + 1]
    seg = plan[HDR + B + J + 1:HDR + B + J + 1 + 3 * ns].reshape(ns, 3)
    return rc, perm, grp, seg, ns


def _check_plan(g, J, perm, grp, seg, ns, cap):
    g = np.asarray(g)
    B = len(g)
    npt.assert_array_equal(perm, np.argsort(g, kind="stable"))            # by group, ascending row within a group
    assert grp[0] == 0 and grp[J] == ns and (np.diff(grp) >= 0).all()
    counts = np.bincount(g, minlength=J) if B else np.zeros(J, int)
    at = 0
    for j in range(J):
        mine = seg[grp[j]:grp[j + 1]]
        assert len(mine) == -(-counts[j] // cap)                          # an empty group has no segment
        for start, length, group in mine:
            assert group == j and start == at and 1 <= length <= cap
            at += length
        if len(mine):
            assert (mine[:-1, 1] == cap).all()                            # only a group's last segment is short
    assert at == B


def test_plan_host_core(lib):
    from bayesic_amd import _ffi
    header = open(_ffi.os.path.join(_ffi.os.path.dirname(_ffi._HERE), "include", "bayesic_hip.h")).read()
    cap = int(__import__("re").search(r"#define BSC_GLM_GROUP_SEG_ROWS (\d+)", header).group(1))
    rs = np.random.RandomState(5)
    # stable order, with empty groups (ids 3 and 6 never occur)
    g = rs.choice([0, 1, 2, 4, 5, 7], size=1003).astype(np.int32)
    rc, perm, grp, seg, ns = _plan(lib, g, 8)
    assert rc == 0 and ns == 6
    _check_plan(g, 8, perm, grp, seg, ns, cap)
    assert grp[3] == grp[4] and grp[6] == grp[7]
    # J = 1: one run, cut at the cap
    g = np.zeros(cap + 5, np.int32)
    rc, perm, grp, seg, ns = _plan(lib, g, 1)
    assert rc == 0 and ns == 2
    _check_plan(g, 1, perm, grp, seg, ns, cap)
    # one group larger than several caps between two small ones: its segments in order
    g = np.concatenate([np.full(7, 2), np.full(3 * cap + 11, 1), np.full(5, 0)]).astype(np.int32)
    g = g[rs.permutation(len(g))]
    rc, perm, grp, seg, ns = _plan(lib, g, 4)
    assert rc == 0 and ns == 1 + 4 + 1 and grp[2] - grp[1] == 4
    _check_plan(g, 4, perm, grp, seg, ns, cap)
    # B = 0
    rc, perm, grp, seg, ns = _plan(lib, np.zeros(0, np.int32), 3)
    assert rc == 0 and ns == 0 and (grp == 0).all()
    # ids outside [0, J): refused, the first offending row named
    for bad, J in ((-1, 5), (5, 5)):
        g = rs.randint(5, size=100).astype(np.int32)
        g[41], g[77] = bad, bad
        rc = _plan(lib, g, J)[0]
        assert rc != 0
        msg = lib.bsc_last_error().decode()
        assert "row 41 has group id %d outside [0,5)" % bad in msg, msg
    # the size query refuses what the plan cannot hold
    assert lib.bsc_glm_group_plan_size(10, 0) == -1 and lib.bsc_glm_group_plan_size(10, 65537) == -1
    assert lib.bsc_glm_group_plan_size(-1, 3) == -1
    assert lib.bsc_glm_group_plan_size(0, 65536) > 0


# ---- the driver: argument errors before any device call -------------------------------------------------------------

class _NoDevice:
    """A context that fails the test when the driver touches it."""

    def __getattr__(self, name):
        raise AssertionError("the driver reached for the device (ctx.%s) before refusing its arguments" % name)


def test_driver_argument_errors_come_before_any_device_call():
    from bayesic_amd.svi import HierGLMReparamSVI
    X, y = torch.zeros((12, 8), dtype=torch.float32), torch.zeros(12, dtype=torch.float32)
    g = torch.zeros(12, dtype=torch.int32)
    ones = torch.ones(12, dtype=torch.float32)
    ctx = _NoDevice()
    with pytest.raises(ValueError, match="mean-field guide only"):
        HierGLMReparamSVI(X, y, g, 3, covariance="full", ctx=ctx)
    with pytest.raises(ValueError, match="link must be"):
        HierGLMReparamSVI(X, y, g, 3, link="probit", ctx=ctx)
    with pytest.raises(ValueError, match="exposure belongs to the Poisson"):
        HierGLMReparamSVI(X, y, g, 3, exposure=ones, ctx=ctx)
    with pytest.raises(ValueError, match="mutually exclusive"):
        HierGLMReparamSVI(X, y, g, 3, link="poisson", exposure=ones, offset=ones, ctx=ctx)
    for J in (0, 65537, 2.5):
        with pytest.raises(ValueError, match="n_groups must be an integer in"):
            HierGLMReparamSVI(X, y, g, J, ctx=ctx)
    with pytest.raises(ValueError, match="prior_precision must be positive"):
        HierGLMReparamSVI(X, y, g, 3, prior_precision=0.0, ctx=ctx)
    with pytest.raises(ValueError, match="a0 and b0"):
        HierGLMReparamSVI(X, y, g, 3, b0=-1.0, ctx=ctx)
    with pytest.raises(ValueError, match="n_samples must be in"):
        HierGLMReparamSVI(X, y, g, 3, n_samples=65, ctx=ctx)
    with pytest.raises(TypeError, match="groups must be int32"):
        HierGLMReparamSVI(X, y, g.long(), 3, ctx=ctx)
    with pytest.raises(ValueError, match=r"groups must be a contiguous \[12\]"):
        HierGLMReparamSVI(X, y, g[:11], 3, ctx=ctx)
    with pytest.raises(ValueError, match="groups is required"):
        HierGLMReparamSVI(X, y, None, 3, ctx=ctx)
    with pytest.raises(ValueError, match=r"weights must be \[12\]"):
        HierGLMReparamSVI(X, y, g, 3, weights=torch.ones((12, 1)), ctx=ctx)
    with pytest.raises(ValueError, match="finite and >= 0"):
        HierGLMReparamSVI(X, y, g, 3, weights=-ones, ctx=ctx)
    with pytest.raises(ValueError, match="lam0 has 5 entries"):
        HierGLMReparamSVI(X, y, g, 3, lam0=np.zeros(5), ctx=ctx)


def test_entry_points_are_declared_and_bound():
    from bayesic_amd import _ffi
    header = open(_ffi.os.path.join(_ffi.os.path.dirname(_ffi._HERE), "include", "bayesic_hip.h")).read()
    for name in ("bsc_glm_group_plan", "bsc_glm_data_pass_groups", "bsc_glm_hier_update"):
        assert "int %s(bsc_ctx* ctx" % name in header and name in _ffi.SIGNATURES
    assert "bsc_glm_group_plan_host" in _ffi.SIGNATURES and "bsc_glm_group_plan_size" in _ffi.SIGNATURES
    # the finish's argument tail is bsc_glm_update's with Bz, J, a0, b0 and Bz_next added
    assert len(_ffi.SIGNATURES["bsc_glm_hier_update"][1]) == len(_ffi.SIGNATURES["bsc_glm_update"][1]) + 5


# ---- the reference stepper on a small hierarchy ---------------------------------------------------------------------

def test_reference_stepper_recovers_the_group_intercepts():
    """N = 20 000, D = 8, J = 20, three hundred full-batch updates at S = 8: the intercept means correlate with the
    generating b, which the zero initial state does not (its correlation is undefined; 0 here).  A sanity check of the
    reference alone; the correlation reached is printed, and only compared with the initial state's."""
    rs = np.random.RandomState(11)
    N, D, J, S, seed, lr = 20000, 8, 20, 8, 3, 0.05
    X = rs.standard_normal((N, D)).astype(np.float32)
    w_true, b_true = rs.standard_normal(D) / 3.0, rs.standard_normal(J)
    g = rs.randint(J, size=N).astype(np.int32)
    y = (rs.uniform(size=N) < 1.0 / (1.0 + np.exp(-(X.astype(np.float64) @ w_true + b_true[g])))).astype(np.float32)
    P = D + J + 1
    lam = ref.init_lam(P)
    m1, m2 = np.zeros_like(lam), np.zeros_like(lam)
    elbos = []
    for t in range(1, 301):
        lam, m1, m2, elbo, _ = ref.step("logistic", lam, m1, m2, t, X, y, g, J, S, seed, float(N), lr)
        elbos.append(elbo)
    corr = float(np.corrcoef(lam[D:D + J], b_true)[0, 1])
    print("correlation of the intercept means with the generating b after 300 updates: %.4f; ELBO %.1f -> %.1f; "
          "zeta mean %.3f (generating precision 1: zeta = 0)" % (corr, elbos[0], elbos[-1], lam[P - 1]))
    assert np.isfinite(lam).all()
    assert corr > 0.0                       # the initial state's intercept means are all zero
    assert elbos[-1] > elbos[0]
