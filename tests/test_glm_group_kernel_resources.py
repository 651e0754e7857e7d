"""Compile-time resource guard for the grouped GLM pass kernels (csrc/bsc_glm_group.hip), as
tests/test_glm_obs_kernel_resources.py keeps for the kernels without group ids (no GPU needed: hipcc cross-compiles for
gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_group_pass_mfma_kernel<logistic>          226, 0, 2        glm_group_pass_mfma_kernel<poisson>          226, 0, 2
    glm_group_pass_kernel<logistic, D == 256>     225, 0, 2        glm_group_pass_kernel<poisson, D == 256>     224, 0, 2
    glm_group_pass_kernel<logistic, D < 256>      227, 0, 2        glm_group_pass_kernel<poisson, D < 256>      225, 0, 2

(the kernels with offset and weight alone: 214 / 212, 221 / 219, 223 / 220: the ids, the gathered intercepts and the
residual store's descriptor cost 4 to 14 registers).  The pass kernels are launched for two waves per SIMD: 256 VGPRs at
most; the guard is the measured count plus 24, capped at 256."""
import os

import pytest

from test_glm_obs_kernel_resources import HIPCC, _check, resources

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_group_pass_mfma_kernelILi0E": 226,
    "glm_group_pass_mfma_kernelILi1E": 226,
    "glm_group_pass_kernelILi0ELb1E": 225,
    "glm_group_pass_kernelILi0ELb0E": 227,
    "glm_group_pass_kernelILi1ELb1E": 224,
    "glm_group_pass_kernelILi1ELb0E": 225,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_glm_group_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_glm_group.hip")
    assert got, "no resource remarks from hipcc for bsc_glm_group.hip"
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_group.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
    # the small kernels behind the pass keep out of scratch too
    for needle in ("glm_group_segment_kernel", "glm_group_sum_kernel", "glm_hier_scalars_kernel",
                   "glm_hier_coord_kernel"):
        matches = [v for k, v in got.items() if needle in k]
        assert len(matches) == 1 and matches[0]["ScratchSize"] == 0, needle
