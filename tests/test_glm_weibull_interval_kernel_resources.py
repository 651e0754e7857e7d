"""Compile-time resource guard for the kernels of the Weibull route with interval and left censoring
(csrc/bsc_glm_weibull_interval.hip), as tests/test_glm_weibull_kernel_resources.py keeps for the kernels without the upper
ends (no GPU needed: hipcc cross-compiles for gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_weibull_itv_pass_mfma_kernel            226, 0, 2
    glm_weibull_itv_pass_kernel<D == 256>       235, 0, 2        glm_weibull_itv_pass_kernel<D < 256>       235, 0, 2

(the kernels without the upper ends: 216, 227, 227).  The pass kernels are launched for two waves per SIMD: 256 VGPRs at
most; the guard is the measured count plus 24, capped at 256.  Every select of the link is flat and sits on its inputs
(csrc/bsc_glm_pass.h, glm_link): with one nested select the 8-row kernels came out with a branch in the loop body, 256
VGPRs and 150 bytes of scratch per lane.

predict_weibull_itv_kernel<chunks of 16 draws, D == 256> (VGPRs; scratch 0 and 2 waves per SIMD for every one; LDS as the
kernels without the upper ends):

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
              107       100                 118       111                 139       130
"""
import os
import shutil

import pytest

from test_glm_obs_kernel_resources import _check, resources

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SOURCE = "bsc_glm_weibull_interval.hip"

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_weibull_itv_pass_mfma_kernelE": 226,
    "glm_weibull_itv_pass_kernelILb1E": 235,
    "glm_weibull_itv_pass_kernelILb0E": 235,
}

# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 107, (1, 0): 100, (2, 1): 118, (2, 0): 111, (4, 1): 139, (4, 0): 130}

# three passes, the slab reduction, six predictive kernels and their sum
N_KERNELS = 11


@pytest.fixture(scope="module")
def got():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources(SOURCE)
    assert out, "no resource remarks from hipcc for %s" % SOURCE
    return out


def test_interval_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            _check(name, r, measured)


def test_interval_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "predict_weibull_itv_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "predict_weibull_itv_kernelILi%dELb%dE" % (nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(got):
    """The slab reduction and the predictive's sum as well."""
    assert len(got) == N_KERNELS, sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
