"""Compile-time resource guard for the ordinal-regression kernels (csrc/bsc_glm_ordinal.hip), as
tests/test_scalar_family_kernel_resources.py keeps for the Weibull ones (no GPU needed: hipcc cross-compiles for gfx950;
only the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_ordinal_pass_mfma_kernel                228, 0, 2
    glm_ordinal_pass_kernel<D == 256>           238, 0, 2        glm_ordinal_pass_kernel<D < 256>           238, 0, 2

(the Weibull kernels: 216, 227, 227; the logistic ones with offset and weight: 214, 221, 223).  The pass kernels are
launched for two waves per SIMD: 256 VGPRs at most; the guard is the measured count plus 24, capped at 256.  What the
ordinal link adds to the logistic one in registers is its seven cutpoint-gradient accumulators; the (draw, class) table
sits in LDS (1 KiB per workgroup: 69 632 and 71 680 bytes with the tiles).

predict_ordinal_kernel<chunks of 16 draws, D == 256> (VGPRs; scratch 0 and 2 waves per SIMD for every one; LDS 88 000,
104 512 and 137 536 bytes for 1, 2 and 4 chunks).  The draws of a row run in a loop, staged through the strip buffer:

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
              128       121                 125       119                 131       117
"""
import os
import shutil

import pytest

from test_glm_obs_kernel_resources import _check, resources

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_ordinal_pass_mfma_kernelE": 228,
    "glm_ordinal_pass_kernelILb1E": 238,
    "glm_ordinal_pass_kernelILb0E": 238,
}

# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 128, (1, 0): 121, (2, 1): 125, (2, 0): 119, (4, 1): 131, (4, 0): 117}

# three passes, the slab reduction, six predictive kernels and their sum
N_KERNELS = 11


@pytest.fixture(scope="module")
def got():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources("bsc_glm_ordinal.hip")
    assert out, "no resource remarks from hipcc for bsc_glm_ordinal.hip"
    return out


def test_glm_ordinal_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_ordinal.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 80 * 1024, "%s: %d bytes of LDS: two workgroups per CU need 80 KiB each" % (name, r["LDS"])


def test_predict_ordinal_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "predict_ordinal_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "predict_ordinal_kernelILi%dELb%dE" % (nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_ordinal.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(got):
    """The slab reduction and the predictive's sum as well."""
    assert len(got) == N_KERNELS, sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
