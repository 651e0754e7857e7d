"""Compile-time resource guard for the Weibull survival kernels (csrc/bsc_glm_weibull.hip), as
tests/test_glm_gamma_kernel_resources.py keeps for the Gamma ones (no GPU needed: hipcc cross-compiles for gfx950; only
the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_weibull_pass_mfma_kernel                216, 0, 2
    glm_weibull_pass_kernel<D == 256>           227, 0, 2        glm_weibull_pass_kernel<D < 256>           227, 0, 2

(the Gamma kernels: 218, 228, 228; the negative-binomial kernels: 220, 245, 245).  The pass kernels are launched for
two waves per SIMD: 256 VGPRs at most; the guard is the measured count plus 24, capped at 256.  The link's selects sit
on its inputs (csrc/bsc_glm_pass.h, glm_link), as the other two per-draw-scalar links' do.

predict_weibull_kernel<chunks of 16 draws, D == 256> (VGPRs; scratch 0 and 2 waves per SIMD for every one; LDS 84 160,
100 672 and 133 696 bytes for 1, 2 and 4 chunks):

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
              100        94                 112       100                 145       124
"""
import os
import shutil

import pytest

from test_glm_obs_kernel_resources import _check, resources

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_weibull_pass_mfma_kernelE": 216,
    "glm_weibull_pass_kernelILb1E": 227,
    "glm_weibull_pass_kernelILb0E": 227,
}

# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 100, (1, 0): 94, (2, 1): 112, (2, 0): 100, (4, 1): 145, (4, 0): 124}

# three passes, the slab reduction, the two finish kernels, six predictive kernels and their sum
N_KERNELS = 13


@pytest.fixture(scope="module")
def got():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources("bsc_glm_weibull.hip")
    assert out, "no resource remarks from hipcc for bsc_glm_weibull.hip"
    return out


def test_glm_weibull_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_weibull.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)


def test_predict_weibull_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "predict_weibull_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "predict_weibull_kernelILi%dELb%dE" % (nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_weibull.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(got):
    """The slab reduction, the two finish kernels and the predictive's sum as well."""
    assert len(got) == N_KERNELS, sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
