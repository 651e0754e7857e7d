"""Compile-time resource guard for the kernels of the Student-t route, csrc/bsc_glm_studentt.hip over the kernel set of
csrc/bsc_scalar_family.h -- tests/test_glm_zip_kernel_resources.py's form for one more unit (no GPU needed: hipcc
cross-compiles for gfx950; only the compiler's resource remarks are read).  This is the first unit whose pass and
predictive kernels are the scalar_par_* templates, which take the family's per-model constant (the degrees of freedom)
as one float behind their other arguments: the unit has those and none of the plain or `upper` pass kernels.

Measured from this compile (VGPRs; scratch 0 bytes per lane and 2 waves per SIMD for every one of the 13 kernels):

    scalar_par_pass_mfma_kernel<GLM_ID 8>              218
    scalar_par_pass_kernel<GLM_ID 8, D == 256>         233
    scalar_par_pass_kernel<GLM_ID 8, D < 256>          233

(the Poisson kernels with offset and weight: 212, 219, 220; the zero-inflated Poisson's: 222, 238, 238 in
tests/test_glm_zip_kernel_resources.py's table).  The pass kernels are launched for two waves per SIMD: 256 VGPRs at most;
the guard is the measured count plus 24, capped at 256.  The link is one log, one division and one reciprocal per
(row, draw) with flat selects on its inputs, and the constant costs no register of its own: it rides in the fourth of the
draw's four.

scalar_par_predict_kernel<PREDICT_ID 10, chunks of 16 draws, D == 256>:

    chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
          103        96                 127       120                 168       168
"""
import os

import pytest

from test_glm_obs_kernel_resources import _check, resources
from test_scalar_family_kernel_resources import HIPCC

SOURCE = "bsc_glm_studentt.hip"
LINK, FAMILY = 8, 10                      # StudentT::GLM_ID and ::PREDICT_ID of csrc/bsc_families.h
# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {"scalar_par_pass_mfma_kernelILi%dEE" % LINK: 218,
                "scalar_par_pass_kernelILi%dELb1EE" % LINK: 233,
                "scalar_par_pass_kernelILi%dELb0EE" % LINK: 233}
# (chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {(1, 1): 103, (1, 0): 96, (2, 1): 127, (2, 0): 120, (4, 1): 168, (4, 0): 168}
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
            assert name.endswith("f"), "%s: the constant is the last argument, one float" % name
            _check(name, r, measured)


def test_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd(got):
    kernels = {k: v for k, v in got.items() if "scalar_par_predict_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (nc, full), measured in PREDICT_KERNELS.items():
        needle = "scalar_par_predict_kernelILi%dELi%dELb%dEE" % (FAMILY, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            assert name.endswith("f"), "%s: the constant is the last argument, one float" % name
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(got):
    """The slab reduction, the two finish kernels and the predictive's sum as well; no plain pass or predictive kernel
    and no `upper` kernel."""
    assert len(got) == N_KERNELS, sorted(got)
    assert not [name for name in got if "scalar_upper_" in name], sorted(got)
    assert not [name for name in got if "scalar_pass_" in name or "scalar_predict_kernel" in name], sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
