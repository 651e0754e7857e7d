"""Compile-time resource guard for the grouped predictive pass (no GPU needed: hipcc cross-compiles for gfx950), as
tests/test_predict_kernel_resources.py keeps for the pass it extends: scratch would pass every parity test and only
show as a slower pass.  Only the compiler's resource remarks are read.

predict_group_kernel<family, chunks of 16 draws, D == 256>, measured from this compile (VGPRs; scratch 0 bytes per
lane, 2 waves per SIMD and 83 904 / 100 416 / 133 440 bytes of LDS at 1 / 2 / 4 chunks for every instantiation):

    family     chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
    logistic            102         94                 114       112                 151       151
    poisson             151        143                 151       149                 175       175

against predict_offset_kernel (tests/test_predict_kernel_resources.py's table, which it shares with predict_kernel to a
few registers) the intercepts cost about 4 registers per chunk and the id one.  The guard is the measured
count plus 24, the headroom tests/test_predict_kernel_resources.py uses; 256 is the ceiling at two waves per SIMD.

The ISA of the D == 256 kernel (logistic, four chunks), read once.  The tile's ids are one buffer_load_dword behind the
next tile's y and offset.  The four 16-byte gathers of the intercepts are issued at the top of the tile's first strip,
ahead of its eight ds_write2_b64, behind an s_waitcnt vmcnt(0) that the shared body already reaches there (the strip
registers are selected against `col >= D` at the end of every iteration, which waits for them).  Nothing is done to the
gathered registers where they are issued; their first readers are behind the tile's last MFMA, under s_waitcnt
vmcnt(11), vmcnt(10), vmcnt(9) and vmcnt(8) -- the eight loads of the next strip and the three scalars of the next tile
stay in flight: the gather does not drain the X prefetch.  (A select on the gathered registers next to the loads did:
the compiler then waited vmcnt(3) .. vmcnt(0) right behind them.)"""
import os

import pytest

from test_predict_kernel_resources import HEADROOM, HIPCC, resources

# (family, chunks, D == 256) -> VGPRs as measured
MEASURED = {
    (1, 1, 1): 102, (1, 1, 0): 94, (1, 2, 1): 114, (1, 2, 0): 112, (1, 4, 1): 151, (1, 4, 0): 151,
    (2, 1, 1): 151, (2, 1, 0): 143, (2, 2, 1): 151, (2, 2, 0): 149, (2, 4, 1): 175, (2, 4, 0): 175,
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_grouped_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_predict_group.hip")
    assert got, "no resource remarks from hipcc for bsc_predict_group.hip"
    kernels = {k: v for k, v in got.items() if "predict_group_kernel" in k}
    assert len(kernels) == len(MEASURED) == 12, sorted(kernels)
    for (fam, nc, full), vgprs in MEASURED.items():
        needle = "predict_group_kernelILi%dELi%dELb%dE" % (fam, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_predict_group.hip (renamed?)" % needle
        for name, r in matches.items():
            print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD, %d bytes of LDS" % (
                name, r["VGPRs"], r["ScratchSize"], r["Occupancy"], r["LDS"]))
            assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
            assert r["VGPRs"] <= vgprs + HEADROOM, "%s: %d VGPRs > %d" % (name, r["VGPRs"], vgprs + HEADROOM)
            assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])
    for small in ("predict_group_sum_kernel", "group_ids_check_kernel"):
        found = [v for k, v in got.items() if small in k]
        assert len(found) == 1 and found[0]["ScratchSize"] == 0, small
