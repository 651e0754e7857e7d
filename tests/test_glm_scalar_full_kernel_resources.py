"""Compile-time resource guard for the full-covariance finish of the regression families with a learned scalar
(csrc/bsc_glm_scalar_full.hip), as tests/test_glm_full_kernel_resources.py keeps for the GLM one (no GPU needed: hipcc
cross-compiles for gfx950; only the compiler's resource remarks are read): a latency-bound kernel that picks up scratch
still passes every parity test and only shows up as a slower update.

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD, static LDS bytes):

    glm_scalar_fullrank_update_kernel        70, 0, 7, 5672

The guard is the measured count plus 24 (tests/test_glm_obs_kernel_resources.py's convention).  Static LDS is the two
rows of L' (Lnew[2][257]), g of the two rows (gs[2][64]), |w_s|^2 (wsq[64], which also carries f_s) and three doubles
(mu' of the two rows, sum rho): 8 (2 * 257 + 2 * 64 + 64 + 3) = 5672 bytes; the budget leaves room for five more
doubles."""
import os

import pytest

from test_glm_obs_kernel_resources import HIPCC, _check, resources

KERNEL = "glm_scalar_fullrank_update_kernel"
VGPRS = 70
LDS_BUDGET = 8 * (2 * 257 + 2 * 64 + 64 + 8)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_unit_holds_one_kernel_without_scratch_within_its_vgpr_and_lds_budget():
    got = resources("bsc_glm_scalar_full.hip")
    assert got, "no resource remarks from hipcc for bsc_glm_scalar_full.hip"
    assert len(got) == 1, sorted(got)
    (name, r), = got.items()
    assert KERNEL in name, name
    _check(name, r, VGPRS)
    assert r["LDS"] <= LDS_BUDGET, "%s: %d bytes of LDS > %d" % (name, r["LDS"], LDS_BUDGET)
