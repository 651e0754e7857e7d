"""Compile-time resource guard for the grouped pass kernels of the families with a learned scalar
(csrc/bsc_glm_scalar_group.hip) and their predictive kernels (csrc/bsc_predict_scalar_group.hip), as
tests/test_glm_group_kernel_resources.py keeps for the logistic and Poisson ones (no GPU needed: hipcc cross-compiles for
gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs; scratch 0 bytes per lane and 2 waves per SIMD for every one):

    glm_scalar_group_pass_...      mfma_kernel     kernel<D == 256>     kernel<D < 256>
    negative binomial  (link 2)        234               250                  250
    Gamma              (link 3)        230               233                  233
    Weibull            (link 4)        230               232                  233

(the negative binomial's 8-row kernel is the one closest to the 256 registers of two waves per SIMD; it stays below
them without a spill, so every instantiation keeps __launch_bounds__(PASS_BLOCK, 2) and none runs at one wave).

    scalar_predict_group_kernel<family, chunks of 16 draws, D == 256>
    family              chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
    negative binomial (3)         157        149                 176       176                 237       237
    Gamma             (4)         105         94                 114       109                 145       136
    Weibull           (5)         106         97                 116       111                 149       141

The guard is the measured count plus 24, capped at 256."""
import os

import pytest

from test_glm_obs_kernel_resources import HIPCC, _check, resources

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_scalar_group_pass_mfma_kernelILi2E": 234,
    "glm_scalar_group_pass_mfma_kernelILi3E": 230,
    "glm_scalar_group_pass_mfma_kernelILi4E": 230,
    "glm_scalar_group_pass_kernelILi2ELb1E": 250,
    "glm_scalar_group_pass_kernelILi2ELb0E": 250,
    "glm_scalar_group_pass_kernelILi3ELb1E": 233,
    "glm_scalar_group_pass_kernelILi3ELb0E": 233,
    "glm_scalar_group_pass_kernelILi4ELb1E": 232,
    "glm_scalar_group_pass_kernelILi4ELb0E": 233,
}

# (family, chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {
    (3, 1, 1): 157, (3, 1, 0): 149, (3, 2, 1): 176, (3, 2, 0): 176, (3, 4, 1): 237, (3, 4, 0): 237,
    (4, 1, 1): 105, (4, 1, 0): 94, (4, 2, 1): 114, (4, 2, 0): 109, (4, 4, 1): 145, (4, 4, 0): 136,
    (5, 1, 1): 106, (5, 1, 0): 97, (5, 2, 1): 116, (5, 2, 0): 111, (5, 4, 1): 149, (5, 4, 0): 141,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_scalar_group_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_glm_scalar_group.hip")
    assert got, "no resource remarks from hipcc for bsc_glm_scalar_group.hip"
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_scalar_group.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
    # the small kernels behind the pass keep out of scratch too
    for needle in ("glm_scalar_group_slab_reduce_kernel", "glm_group_segment_kernel", "glm_group_sum_kernel",
                   "glm_scalar_hier_scalars_kernel", "glm_scalar_hier_coord_kernel"):
        matches = [v for k, v in got.items() if needle in k]
        assert len(matches) == 1 and matches[0]["ScratchSize"] == 0, needle


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_scalar_group_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_predict_scalar_group.hip")
    assert got, "no resource remarks from hipcc for bsc_predict_scalar_group.hip"
    kernels = {k: v for k, v in got.items() if "scalar_predict_group_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (fam, nc, full), measured in PREDICT_KERNELS.items():
        needle = "scalar_predict_group_kernelILi%dELi%dELb%dE" % (fam, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_predict_scalar_group.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])
    sums = [v for k, v in got.items() if "scalar_predict_group_sum_kernel" in k]
    assert len(sums) == 1 and sums[0]["ScratchSize"] == 0
