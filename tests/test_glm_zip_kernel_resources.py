"""Compile-time resource guard for the kernels of the zero-inflated Poisson route, csrc/bsc_glm_zip.hip over the kernel set
of csrc/bsc_scalar_family.h -- tests/test_glm_lognormal_kernel_resources.py's form for one more unit (no GPU needed: hipcc
cross-compiles for gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs; scratch 0 bytes per lane and 2 waves per SIMD for every one of the 13 kernels):

    scalar_pass_mfma_kernel<GLM_ID 7>              222
    scalar_pass_kernel<GLM_ID 7, D == 256>         238
    scalar_pass_kernel<GLM_ID 7, D < 256>          238

(the Poisson kernels with offset and weight: 212, 219, 220; the negative binomial's: 220, 245, 245 in
tests/test_scalar_family_kernel_resources.py's table).  The pass kernels are launched for two waves per SIMD: 256 VGPRs at
most; the guard is the measured count plus 24, capped at 256.  What keeps the 8-row kernels there: the branch of a row is
an indicator on y == 0 that MULTIPLIES both branches' terms.  With a select between the two branches' results
(zero ? a : b) the compiler branches around the zero row's evaluation, the loop body splits, and both 8-row kernels
came out at 256 VGPRs with 140 and 144 bytes of scratch per lane.

scalar_predict_kernel<PREDICT_ID 9, chunks of 16 draws, D == 256> (with the float64 lnGamma(y + 1) of ROW_LGAMMA, as the
negative binomial's: 151 .. 221):

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
          149       143                 173       166                 219       219
"""
import os

import pytest

from test_glm_obs_kernel_resources import _check, resources
from test_scalar_family_kernel_resources import HIPCC

SOURCE = "bsc_glm_zip.hip"
LINK, FAMILY = 7, 9                       # ZeroInflPoisson::GLM_ID and ::PREDICT_ID of csrc/bsc_families.h
# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {"scalar_pass_mfma_kernelILi%dEE" % LINK: 222,
                "scalar_pass_kernelILi%dELb1EE" % LINK: 238,
                "scalar_pass_kernelILi%dELb0EE" % LINK: 238}
# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 149, (1, 0): 143, (2, 1): 173, (2, 0): 166, (4, 1): 219, (4, 0): 219}
N_KERNELS = 13       # three passes, the slab reduction, the two finish kernels, six predictive kernels and their sum


@pytest.fixture(scope="module")
def got():
    """kernel name -> the compiler's resource remarks"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources(SOURCE)
    assert out, "no resource remarks from hipcc for %s" % SOURCE
    return out


def test_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            _check(name, r, measured)


def test_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "scalar_predict_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "scalar_predict_kernelILi%dELi%dELb%dEE" % (FAMILY, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(got):
    """The slab reduction, the two finish kernels and the predictive's sum as well; no `upper` kernel."""
    assert len(got) == N_KERNELS, sorted(got)
    assert not [name for name in got if "scalar_upper_" in name], sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
