"""Compile-time resource guard for the kernels of the families with a learned log-scalar behind the weights, one
translation unit each over the kernel set of csrc/bsc_scalar_family.h: csrc/bsc_glm_nb.hip, csrc/bsc_glm_gamma.hip,
csrc/bsc_glm_weibull.hip and, with the upper ends, csrc/bsc_glm_weibull_interval.hip -- as
tests/test_glm_obs_kernel_resources.py keeps for the passes with offsets and weights (no GPU needed: hipcc
cross-compiles for gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs; scratch 0 bytes per lane and 2 waves per SIMD for every one):

    unit                          scalar_pass_mfma_kernel    scalar_pass_kernel<D == 256>    scalar_pass_kernel<D < 256>
    bsc_glm_nb                              220                          245                            245
    bsc_glm_gamma                           218                          228                            228
    bsc_glm_weibull                         216                          227                            227
    bsc_glm_weibull_interval (upper)        226                          235                            235

(the logistic kernels with offset and weight: 214, 221, 223; the Poisson ones: 212, 219, 220).  The pass kernels are
launched for two waves per SIMD: 256 VGPRs at most; the guard is the measured count plus 24, capped at 256.  What keeps
the 8-row kernels there: every select of a link is flat and sits on its inputs (csrc/bsc_glm_pass.h, glm_link).  With a
select on the results the compiler branches around the negative binomial's lnGamma / psi evaluation, the loop body
splits, and both instantiations spill (256 VGPRs, over 100 bytes each); with one nested select the interval link's 8-row
kernels came out with a branch in the loop body, 256 VGPRs and 150 bytes of scratch per lane.

scalar_predict_kernel<family, chunks of 16 draws, D == 256> (the interval unit: scalar_upper_predict_kernel; LDS of the
Weibull ones 84 160, 100 672 and 133 696 bytes for 1, 2 and 4 chunks):

    unit                          chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
    bsc_glm_nb                              151       143                 173       166                 221       221
    bsc_glm_gamma                            99        91                 110        98                 141       120
    bsc_glm_weibull                         100        94                 112       100                 145       124
    bsc_glm_weibull_interval                107       100                 118       111                 139       130
"""
import os
import shutil

import pytest

from test_glm_obs_kernel_resources import _check, resources

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# unit -> (LINK of csrc/bsc_glm_pass.h, FAMILY of csrc/bsc_predict_pass.h, "upper_" for the kernels with the upper ends,
#          VGPRs as measured of the MFMA pass and the 8-row pass with D == 256 and D < 256,
#          (chunks, D == 256) -> VGPRs as measured of the predictive,
#          kernels in all: three passes, the slab reduction, the two finish kernels (not in the interval unit), six
#          predictive kernels and their sum)
UNITS = {
    "bsc_glm_nb": (2, 3, "", (220, 245, 245),
                   {(1, 1): 151, (1, 0): 143, (2, 1): 173, (2, 0): 166, (4, 1): 221, (4, 0): 221}, 13),
    "bsc_glm_gamma": (3, 4, "", (218, 228, 228),
                      {(1, 1): 99, (1, 0): 91, (2, 1): 110, (2, 0): 98, (4, 1): 141, (4, 0): 120}, 13),
    "bsc_glm_weibull": (4, 5, "", (216, 227, 227),
                        {(1, 1): 100, (1, 0): 94, (2, 1): 112, (2, 0): 100, (4, 1): 145, (4, 0): 124}, 13),
    "bsc_glm_weibull_interval": (4, 5, "upper_", (226, 235, 235),
                                 {(1, 1): 107, (1, 0): 100, (2, 1): 118, (2, 0): 111, (4, 1): 139, (4, 0): 130}, 11),
}


@pytest.fixture(scope="module", params=sorted(UNITS))
def unit(request):
    """(the unit's row of UNITS, its source file, kernel name -> the compiler's resource remarks)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    source = request.param + ".hip"
    got = resources(source)
    assert got, "no resource remarks from hipcc for %s" % source
    return UNITS[request.param], source, got


def test_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd(unit):
    (link, _, upper, (mfma, full, rest), _, _), source, got = unit
    # mangled-name substring -> VGPRs as measured
    kernels = {"scalar_%spass_mfma_kernelILi%dEE" % (upper, link): mfma,
               "scalar_%spass_kernelILi%dELb1EE" % (upper, link): full,
               "scalar_%spass_kernelILi%dELb0EE" % (upper, link): rest}
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(kernels), sorted(got)
    for needle, measured in kernels.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, source)
        for name, r in matches.items():
            _check(name, r, measured)


def test_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd(unit):
    (_, family, upper, _, measured_of, _), source, got = unit
    stem = "scalar_%spredict_kernel" % upper
    kernels = {k: v for k, v in got.items() if stem in k}
    assert len(kernels) == len(measured_of), sorted(kernels)
    for (nc, full), measured in measured_of.items():
        needle = "%sILi%dELi%dELb%dEE" % (stem, family, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, source)
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch_at_two_waves(unit):
    """The slab reduction, the two finish kernels and the predictive's sum as well: a unit has the kernels of the host
    templates it calls and no other (no `upper` kernel without the upper ends, no finish in the interval unit)."""
    (_, _, upper, _, _, n_kernels), source, got = unit
    assert len(got) == n_kernels, sorted(got)
    assert all(("scalar_upper_" in name) == bool(upper) for name in got if "pass" in name or "predict_kernel" in name), \
        sorted(got)
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
