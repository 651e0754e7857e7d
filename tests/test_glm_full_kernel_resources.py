"""Compile-time resource guard for the full-covariance GLM finish (no GPU needed: hipcc cross-compiles for gfx950), as
tests/test_glm_kernel_resources.py keeps for the mean-field one: a latency-bound kernel that picks up scratch still
passes every parity test and only shows up as a slower update.

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_fullrank_update_kernel               70, 0, 7"""
import os

import pytest

from test_glm_kernel_resources import HIPCC, resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_glm_fullrank_finish_uses_no_scratch_and_at_most_128_vgprs():
    got = resources("bsc_glm_full.hip")
    assert got, "no resource remarks from hipcc for bsc_glm_full.hip"
    finish = {k: v for k, v in got.items() if "glm_fullrank_update_kernel" in k}
    assert len(finish) == 1, "glm_fullrank_update_kernel found %d times in bsc_glm_full.hip (renamed?)" % len(finish)
    for name, r in finish.items():
        print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD" % (name, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
        assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
        assert r["VGPRs"] <= 128, "%s: %d VGPRs > 128" % (name, r["VGPRs"])
