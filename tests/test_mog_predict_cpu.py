"""The posterior predictive of the mixture (csrc/bsc_mog_predict.hip) without a device: the float64 restatement of
tests/_mog_predict_ref.py against scipy, the properties the device suite leans on, and the argument checks of
MoGNatGradSVI.predict / heldout_lpd / predictive_params that run before anything reaches the device.

MEASURED (float64, this file): reference against scipy.stats.t 1.1e-13 at most over the parity cases; the K = 3 predictive
integrates to 1 within 1e-9; Student-t against the Gaussian plug-in 1.4e-1, 1.4e-3, 1.4e-5 nats at a x 1e2, 1e4, 1e6; at
a = 1e5 the plain float32 log(1 + u) is off by 2.2e-3 of the bound quantity (112 x the tolerance of 2e-5), the corrected
quotient by 7.6e-8; near-tie shares 0 to 0.12 % (cap 1 %); held-out lpd per row -8.7185 (K = 5), -13.6218 (K = 2), -15.4469
(K = 1)."""
import numpy as np
import pytest

import _mixture_ref as mr
import _mog_predict_ref as pr
from oracle import svi


def test_reference_matches_scipy_student_t_component_by_component():
    worst = 0.0
    for N, D, K in [s for s in pr.PARITY_SHAPES if 0 < s[0] <= 5000]:
        X, eta = pr.fitted_case(N, D, K)
        Pt, c = pr.predictive_table(eta, K, D)
        x = X.astype(np.float64)
        m, q, h = Pt[:, :D], Pt[:, D:2 * D], Pt[:, 2 * D:]
        L = c[None] - (h[None] * np.log1p(q[None] * (x[:, None, :] - m[None]) ** 2)).sum(axis=2)
        want = pr.student_t_logits(X, eta, K, D)
        worst = max(worst, float(np.abs(L - want).max()))
        np.testing.assert_allclose(L, want, rtol=0, atol=1e-11)
    print("reference against scipy.stats.t: %.2e" % worst)


def test_table_of_the_reference_is_what_logits_reads():
    """logits() on the float32 table differs from the float64 form by the table's rounding only."""
    X, eta, Pt, c, ref = pr.parity_reference(1003, 16, 64)
    want = pr.student_t_logits(X, eta, 64, 16)
    assert np.abs(ref["L"] - want).max() <= 4 * 2.0 ** -24 * ref["B"].max()


def test_predictive_integrates_to_one():
    K, D = 3, 1
    eta = pr.pack(np.array([3.0, 9.0, 5.0]), np.array([[-4.0], [0.5], [6.0]]), np.array([[2.0], [5.0], [9.0]]),
                  np.array([[3.0], [4.5], [8.0]]), np.array([[2.0], [9.0], [4.0]]))
    x = np.linspace(-400.0, 400.0, 1600001)
    p = np.exp(pr.student_t_logits(x[:, None], eta, K, D)).sum(axis=1)
    total = float(((p[1:] + p[:-1]) * 0.5 * np.diff(x)).sum())
    print("integral %.9f" % total)
    assert abs(total - 1.0) < 1e-5


def test_predictive_tends_to_the_gaussian_plug_in_mixture():
    """a -> infinity at fixed b / a: St(m, b (kappa + 1) / (a kappa), 2a) -> N(m, (b / a)(kappa + 1) / kappa)."""
    rs = np.random.RandomState(11)
    K, D = 4, 3
    alpha, m = rs.uniform(1, 9, K), rs.standard_normal((K, D)) * 3
    kappa, a, b = rs.uniform(5, 50, (K, D)), rs.uniform(2, 4, (K, D)), rs.uniform(1, 5, (K, D))
    X = (m[rs.randint(K, size=500)] + rs.standard_normal((500, D)))
    var = (b / a) * (kappa + 1.0) / kappa
    gauss = np.log(alpha / alpha.sum())[None] + (-0.5 * np.log(2 * np.pi * var)[None]
                                                 - 0.5 * (X[:, None, :] - m[None]) ** 2 / var[None]).sum(axis=2)
    want = np.logaddexp.reduce(gauss, axis=1)
    gaps = []
    for s in (1e2, 1e4, 1e6):
        L = pr.student_t_logits(X, pr.pack(alpha, m, kappa, a * s, b * s), K, D)
        gaps.append(float(np.abs(np.logaddexp.reduce(L, axis=1) - want).max()))
    print("Student-t against the Gaussian plug-in:", gaps)
    assert gaps[1] < gaps[0] / 50 and gaps[2] < gaps[1] / 50 and gaps[2] < 1e-4      # (the gap goes as 1 / a)


def test_float32_chain_needs_the_corrected_log1p():
    """At a = 1e5 the plain float32 log(1 + u) misses 2e-5 of the bound quantity, the corrected quotient meets it."""
    X, eta = pr.precision_case()
    K, D = 8, 16
    Pt, c = pr.table_f32(eta, K, D)
    ref = pr.predict(X, Pt, c)
    m, q, h = Pt[:, :D], Pt[:, D:2 * D], Pt[:, 2 * D:]
    d = (X[:, None, :] - m[None]).astype(np.float32)
    u = (q[None] * (d * d).astype(np.float32)).astype(np.float32)
    worst = {}
    for corrected in (False, True):
        t = (h[None].astype(np.float64) * pr.log1p_f32(u, corrected).astype(np.float64)).sum(axis=2)
        worst[corrected] = float((np.abs(c.astype(np.float64)[None] - t - ref["L"]) / ref["B"]).max())
    print("error over bound quantity: plain %.2e, corrected %.2e (tolerance %.0e)" % (worst[False], worst[True], pr.EPS))
    assert worst[False] > pr.EPS
    assert worst[True] <= pr.EPS


def test_grid_restatement_at_256_cus():
    cu = 256
    assert [pr.rows_for(it, cu) for it in (1, 2, 3)] == [69, 262213, 524357]
    for it in (1, 2, 3):
        g = pr.grid(pr.rows_for(it, cu), cu)
        assert g["n_iter"] == it, g
        assert g["n_tiles"] == (it - 1) * 4096 + 2
    assert pr.grid(0, cu) == dict(n_tiles=0, n_iter=0, waves=0, n_blocks=0)
    assert pr.grid(4096 * 64, cu) == dict(n_tiles=4096, n_iter=1, waves=4096, n_blocks=1024)
    assert pr.grid(4096 * 64 + 1, cu) == dict(n_tiles=4097, n_iter=2, waves=2049, n_blocks=513)
    assert pr.grid(10_000_000, cu) == dict(n_tiles=156250, n_iter=39, waves=4007, n_blocks=1002)


def test_near_tie_share_of_every_labelled_data_set_is_under_its_cap():
    shares = {}
    for s in pr.PARITY_SHAPES:
        if s[0]:
            shares[s] = float(pr.parity_reference(*s)[4]["tie"].mean())
    X, eta = pr.precision_case()
    shares["precision"] = float(pr.predict(X, *pr.table_f32(eta, 8, 16))["tie"].mean())
    Xe = mr.estep_exact_data(4101, 64, 16)[0]
    shares["exact"] = float(pr.predict(Xe, *pr.table_f32(pr.exact_eta(64, 16), 64, 16))["tie"].mean())
    for K in (1, 2, 5):
        held = pr.cluster_data()[1]
        shares["clusters K=%d" % K] = float(pr.predict(held, *pr.table_f32(pr.cluster_fit(K), K, 5))["tie"].mean())
    print(shares)
    for name, share in shares.items():
        assert share < pr.TIE_CAP, (name, share)


def test_exact_eta_labels_the_exact_data():
    X, _, _, labels, _ = mr.estep_exact_data(4101, 64, 16)
    ref = pr.predict(X, *pr.table_f32(pr.exact_eta(64, 16), 64, 16))
    assert (ref["label"] == labels).all() and not ref["tie"].any()


def test_heldout_lpd_orders_the_fits_by_the_number_of_components():
    held = pr.cluster_data()[1]
    lpd = {K: pr.heldout_lpd64(pr.cluster_fit(K), K, held) for K in (1, 2, 5)}
    print("held-out lpd per row:", lpd)
    assert lpd[5] - lpd[2] >= pr.MARGIN_5_OVER_2
    assert lpd[5] - lpd[1] >= pr.MARGIN_5_OVER_1
    assert lpd[5] - lpd[2] < pr.MARGIN_5_OVER_2 + 0.01 and lpd[5] - lpd[1] < pr.MARGIN_5_OVER_1 + 0.01   # as recorded


class _NoDevice:
    """Stands where the context would: any use of it is a device call the check should have come before."""

    def __getattr__(self, name):
        raise AssertionError("the device was reached (ctx.%s)" % name)


def _model(K, D):
    from bayesic_amd.svi.mog import MoGNatGradSVI
    model = object.__new__(MoGNatGradSVI)
    model.K, model.D, model.ctx = K, D, _NoDevice()
    return model


@pytest.mark.parametrize("K, D", [(65, 4), (8, 17)])
def test_models_past_the_limits_are_refused_before_any_device_call(K, D):
    model = _model(K, D)
    for call in (lambda: model.predict(np.zeros((3, D), np.float32)),
                 lambda: model.predict(np.zeros((3, D), np.float32), responsibilities=True),
                 lambda: model.heldout_lpd(np.zeros((3, D), np.float32))):
        with pytest.raises(NotImplementedError, match=r"K <= 64 components and D <= 16 columns"):
            call()


def test_rows_are_checked_before_any_device_call():
    import torch
    model = _model(8, 4)
    with pytest.raises(ValueError, match="5 columns, the model has D=4"):
        model.predict(np.zeros((3, 5), np.float32))
    with pytest.raises(ValueError, match="5 columns, the model has D=4"):
        model.heldout_lpd(np.zeros((3, 5)))
    with pytest.raises(ValueError, match=r"\[N, D\] array"):
        model.predict(np.zeros(4, np.float32))
    with pytest.raises(ValueError, match="row-major float32"):
        model.predict(torch.zeros((3, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="row-major float32"):
        model.heldout_lpd(torch.zeros((4, 3)).t())
    with pytest.raises(AssertionError, match="device was reached"):       # (the stand-in does what it is there for)
        model.predictive_params()


def test_reference_fit_uses_the_oracle_layout():
    eta = pr.cluster_fit(2)
    alpha, m, kappa, a, b = svi.mog_unpack(eta, 2, 5)
    np.testing.assert_allclose(pr.pack(alpha, m, kappa, a, b), eta, rtol=1e-12)
    assert (b > 0).all() and abs(alpha.sum() - (2 + 3000)) < 1e-6
