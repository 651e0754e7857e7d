"""Compile-time resource guard for the negative-binomial kernels (csrc/bsc_glm_nb.hip), as
tests/test_glm_obs_kernel_resources.py keeps for the passes with offsets and weights (no GPU needed: hipcc
cross-compiles for gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_nb_pass_mfma_kernel                     220, 0, 2
    glm_nb_pass_kernel<D == 256>                245, 0, 2        glm_nb_pass_kernel<D < 256>                245, 0, 2

(the logistic kernels with offset and weight: 214, 221, 223).  The pass kernels are launched for two waves per SIMD: 256
VGPRs at most; the guard is the measured count plus 24, capped at 256.  What keeps the 8-row kernels there: the link's
selects sit on its inputs (csrc/bsc_glm_pass.h, glm_link) -- with a select on the results the compiler branches around
the lnGamma / psi evaluation, the loop body splits, and both instantiations spill (256 VGPRs, over 100 bytes each).

predict_nb_kernel<chunks of 16 draws, D == 256> (VGPRs; scratch 0 and 2 waves per SIMD for every one):

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
              151       143                 173       166                 221       221
"""
import os
import shutil

import pytest

from test_glm_obs_kernel_resources import _check, resources

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_nb_pass_mfma_kernelE": 220,
    "glm_nb_pass_kernelILb1E": 245,
    "glm_nb_pass_kernelILb0E": 245,
}

# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 151, (1, 0): 143, (2, 1): 173, (2, 0): 166, (4, 1): 221, (4, 0): 221}


@pytest.fixture(scope="module")
def got():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources("bsc_glm_nb.hip")
    assert out, "no resource remarks from hipcc for bsc_glm_nb.hip"
    return out


def test_glm_nb_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_nb.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)


def test_predict_nb_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "predict_nb_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "predict_nb_kernelILi%dELb%dE" % (nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_nb.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_no_kernel_of_the_translation_unit_uses_scratch(got):
    """The slab reduction and the two finish kernels as well."""
    assert len(got) == 13, sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
