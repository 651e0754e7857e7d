"""The host helpers of bayesic_amd/svi/_reparam_base.py against the packing of tests/_glm_full_ref.py (numpy only):
the full layout lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal, rho_i in the diagonal slots] is
what every full-covariance driver, the predictive draws and the finishes agree on; and first_draw, the one transform from
noise to draws, against the two expressions the drivers and svi/predict.py wrote out before they shared it."""
import importlib.util
import math
import os

import numpy as np
import numpy.testing as npt
import pytest

import _glm_full_ref as ref

# the module by its path: its helpers are pure numpy, and importing the package would bring torch in
_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayesic_amd", "svi", "_reparam_base.py")
_spec = importlib.util.spec_from_file_location("_reparam_base_under_test", _PATH)
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)
default_lam0, full_size, rho_of_full, unpack_full = base.default_lam0, base.full_size, base.rho_of_full, base.unpack_full

SIZES = [1, 4, 5, 257]


def _factor(P, seed):
    rng = np.random.default_rng(seed)
    L = np.tril(rng.standard_normal((P, P)))
    d = np.arange(P)
    L[d, d] = np.exp(rng.uniform(-3.0, 1.0, P))   # a positive diagonal: e^{rho}
    return rng.standard_normal(P), L


@pytest.mark.parametrize("P", SIZES)
def test_unpack_full_inverts_the_reference_packing(P):
    mu, L = _factor(P, 7 + P)
    lam = ref.pack(mu, L)
    assert lam.shape == (full_size(P),) == (ref.n_lam(P),)
    got_mu, got_L = unpack_full(lam, P)
    npt.assert_array_equal(got_mu, mu)
    # the off-diagonal entries travel untouched; the diagonal goes through log and exp
    off = ~np.eye(P, dtype=bool)
    npt.assert_array_equal(got_L[off], L[off])
    npt.assert_allclose(np.diag(got_L), np.diag(L), rtol=4 * np.finfo(np.float64).eps)
    npt.assert_array_equal(ref.pack(got_mu, got_L)[:P], lam[:P])
    ref_mu, ref_L = ref.unpack(lam, P)
    npt.assert_array_equal(got_mu, ref_mu)
    npt.assert_array_equal(got_L, ref_L)


@pytest.mark.parametrize("P", SIZES)
def test_rho_of_full_reads_the_diagonal_slots(P):
    mu, L = _factor(P, 11 + P)
    lam = ref.pack(mu, L)
    rho = rho_of_full(lam, P)
    npt.assert_array_equal(rho, lam[ref.diag_slots(P)])
    npt.assert_allclose(rho, np.log(np.diag(L)), rtol=0, atol=4 * np.finfo(np.float64).eps)
    npt.assert_array_equal(np.exp(rho), np.diag(unpack_full(lam, P)[1]))


@pytest.mark.parametrize("P", SIZES)
def test_default_lam0_puts_log_tenth_on_exactly_the_diagonal_slots(P):
    full = default_lam0(P, "full")
    assert full.shape == (full_size(P),) and full.dtype == np.float64
    want = np.zeros(full_size(P))
    want[ref.diag_slots(P)] = math.log(0.1)
    npt.assert_array_equal(full, want)
    npt.assert_array_equal(full, ref.init_lam(P))
    assert np.count_nonzero(full) == P
    diag = default_lam0(P, "diag")
    npt.assert_array_equal(diag, np.concatenate([np.zeros(P), np.full(P, math.log(0.1))]))
    # the two defaults are the same guide
    npt.assert_array_equal(ref.from_mean_field(diag, P), full)


@pytest.mark.parametrize("P", SIZES)
def test_first_draw_is_the_two_expressions_bit_for_bit(P):
    rng = np.random.default_rng(13 + P)
    S = 5
    eps = rng.standard_normal((S, P))
    lam = rng.standard_normal(2 * P)
    npt.assert_array_equal(base.first_draw(lam, eps, P, "diag"), lam[None, :P] + np.exp(lam[None, P:]) * eps)
    lam = 0.5 * rng.standard_normal(full_size(P))
    mu, L = unpack_full(lam, P)
    z = base.first_draw(lam, eps, P, "full")
    npt.assert_array_equal(z, mu[None, :] + eps @ L.T)
    assert z.dtype == np.float64 and z.shape == (S, P)
    # the drivers hand over the first P columns of bsc_blr_noise's [S, P + 1] rows as a view
    wide = rng.standard_normal((S, P + 1))
    npt.assert_array_equal(base.first_draw(lam, wide[:, :P], P, "full"), mu[None, :] + wide[:, :P] @ L.T)
