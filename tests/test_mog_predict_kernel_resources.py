"""Compile-time resource guard for the kernels of the mixture's predictive pass, csrc/bsc_mog_predict.hip --
tests/test_glm_zip_kernel_resources.py's form for one more unit (no GPU needed: hipcc cross-compiles for gfx950; only the
compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD, LDS bytes per workgroup):

    mog_predict_kernel<D == 16, with R>        98, 0, 2, 66 592        (launch bounds: 2 waves per SIMD -- the LDS's limit)
    mog_predict_kernel<D == 16, without R>     61, 0, 8,     32        (launch bounds: 4)
    mog_predict_kernel<D < 16,  with R>        42, 0, 2, 66 592
    mog_predict_kernel<D < 16,  without R>     34, 0, 7,     32
    mog_predictive_params_kernel               95, 0, 5
    mog_predict_sum_kernel                     10, 0, 8

What keeps the pass kernels there: the loop over the components carries a running maximum, sum and argmax, not an array of
logits (one indexed by the loop counter lives in scratch), and a component's table [m | q | h] comes through uniform
(scalar) loads, so it takes no vector register.  The guard is the measured count plus 24."""
import os

import pytest

from test_glm_obs_kernel_resources import _check, resources
from test_scalar_family_kernel_resources import HIPCC

SOURCE = "bsc_mog_predict.hip"
# (D == 16, with R) -> (VGPRs as measured, waves per SIMD the launch bounds ask for)
PASS_KERNELS = {(1, 1): (98, 2), (1, 0): (61, 4), (0, 1): (42, 2), (0, 0): (34, 4)}
N_KERNELS = 6        # four passes, the parameter kernel and the sum of the workgroups' partials


@pytest.fixture(scope="module")
def got():
    """kernel name -> the compiler's resource remarks"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = resources(SOURCE)
    assert out, "no resource remarks from hipcc for %s" % SOURCE
    return out


def test_pass_kernels_use_no_scratch_and_keep_their_occupancy(got):
    kernels = {k: v for k, v in got.items() if "mog_predict_kernel" in k}
    assert len(kernels) == len(PASS_KERNELS), sorted(kernels)
    for (full, with_r), (measured, waves) in PASS_KERNELS.items():
        needle = "mog_predict_kernelILb%dELb%dEE" % (full, with_r)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in %s (renamed?)" % (needle, SOURCE)
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["Occupancy"] >= waves, "%s: %d waves per SIMD, launch bounds ask for %d" % (name, r["Occupancy"], waves)
            assert r["LDS"] <= 80 * 1024, "%s: %d bytes of LDS (two workgroups a CU)" % (name, r["LDS"])


def test_every_kernel_of_the_translation_unit_is_there_without_scratch(got):
    assert len(got) == N_KERNELS, sorted(got)
    assert len([k for k in got if "mog_predictive_params_kernel" in k]) == 1
    assert len([k for k in got if "mog_predict_sum_kernel" in k]) == 1
    for name, r in got.items():
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
