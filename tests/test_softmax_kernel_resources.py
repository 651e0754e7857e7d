"""Compile-time resource guard for the softmax-regression kernels (no GPU needed: hipcc cross-compiles for gfx950),
built as tests/test_glm_kernel_resources.py is: a streaming kernel that picks up scratch still passes every parity
test and only shows up as a slower benchmark.

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    softmax_pass_kernel            256, 0, 2
    softmax_predict_kernel         230, 0, 2
    softmax_slab_reduce_kernel      24, 0, 8
    softmax_predict_sum_kernel       8, 0, 8

Both pass kernels are launched for two waves per SIMD (the grid is sized to those slots and two workgroups' LDS fill
a CU): 256 VGPRs at most.  The data pass sits AT that limit (64 accumulator registers for the sixteen-column backward
next to the 64 of the draws and the 64 of the prefetched tile), so its cap is the limit itself and the scratch check
is the one that matters; the predictive kernel gets the usual margin."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel name -> (VGPRs as measured, max VGPRs, min waves per SIMD)
KERNELS = {
    "softmax_pass_kernel": (256, 256, 2),
    "softmax_predict_kernel": (230, 256, 2),
    "softmax_slab_reduce_kernel": (24, 64, 8),
    "softmax_predict_sum_kernel": (8, 64, 8),
}


def resources(source):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize",
           "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-c",
           os.path.join(ROOT, "bayesic_amd", "csrc", source), "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"\s(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_softmax_kernels_use_no_scratch_and_keep_their_waves_per_simd():
    got = resources("bsc_softmax.hip")
    assert got, "no resource remarks from hipcc for bsc_softmax.hip"
    for needle, (_, max_vgpr, min_occ) in KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_softmax.hip (renamed?)" % needle
        for name, r in matches.items():
            print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD" % (name, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
            assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
            assert r["VGPRs"] <= max_vgpr, "%s: %d VGPRs > %d" % (name, r["VGPRs"], max_vgpr)
            assert r["Occupancy"] >= min_occ, "%s: %d waves per SIMD" % (name, r["Occupancy"])
