"""Compile-time resource guard for the GLM pass kernels (no GPU needed: hipcc cross-compiles for gfx950), as
tests/test_kernel_resources.py keeps for the other hot kernels: a streaming kernel that picks up scratch still passes
every parity test and only shows up as a slower benchmark.

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_pass_mfma_kernel<logistic>          200, 0, 2        glm_pass_mfma_kernel<poisson>          198, 0, 2
    glm_pass_kernel<logistic, D == 256>     216, 0, 2        glm_pass_kernel<poisson, D == 256>     216, 0, 2
    glm_pass_kernel<logistic, D < 256>      221, 0, 2        glm_pass_kernel<poisson, D < 256>      216, 0, 2
    glm_update_kernel                        72, 0, 7

The pass kernels are launched for two waves per SIMD (pass_grid sizes the grid to those slots): 256 VGPRs at most."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# mangled-name substring -> (VGPRs as measured, max VGPRs, min waves per SIMD)
PASS_KERNELS = {
    "glm_pass_mfma_kernelILi0E": (200, 224, 2),
    "glm_pass_mfma_kernelILi1E": (198, 224, 2),
    "glm_pass_kernelILi0ELb1E": (216, 240, 2),
    "glm_pass_kernelILi0ELb0E": (221, 240, 2),
    "glm_pass_kernelILi1ELb1E": (216, 240, 2),
    "glm_pass_kernelILi1ELb0E": (216, 240, 2),
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
def test_glm_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_glm.hip")
    assert got, "no resource remarks from hipcc for bsc_glm.hip"
    for needle, (_, max_vgpr, min_occ) in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm.hip (renamed?)" % needle
        for name, r in matches.items():
            print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD" % (name, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
            assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
            assert r["VGPRs"] <= max_vgpr, "%s: %d VGPRs > %d" % (name, r["VGPRs"], max_vgpr)
            assert r["Occupancy"] >= min_occ, "%s: %d waves per SIMD" % (name, r["Occupancy"])
    finish = [v for k, v in got.items() if "glm_update_kernel" in k]
    assert len(finish) == 1 and finish[0]["ScratchSize"] == 0 and finish[0]["VGPRs"] <= 128
