"""Compile-time resource guard for the predictive pass (no GPU needed: hipcc cross-compiles for gfx950), as
tests/test_glm_kernel_resources.py keeps for the GLM pass: scratch would pass every parity test and only show as a
slower pass.  Only the compiler's resource remarks are read.

predict_kernel<family, chunks of 16 draws, D == 256>, measured from this compile (VGPRs; scratch 0 bytes per lane and
2 waves per SIMD -- 512-thread workgroups, one per CU by LDS -- for every instantiation):

    family     chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
    gaussian             96         87                 107        96                 137       117
    logistic             94         87                 107       100                 132       132
    poisson             143        141                 143       137                 156       156

The kernel is launched for two waves per SIMD: 256 VGPRs at most; the guard is the measured count plus 24, the
headroom tests/test_glm_kernel_resources.py uses."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADROOM = 24

# (family, chunks, D == 256) -> VGPRs as measured
MEASURED = {
    (0, 1, 1): 96, (0, 1, 0): 87, (0, 2, 1): 107, (0, 2, 0): 96, (0, 4, 1): 137, (0, 4, 0): 117,
    (1, 1, 1): 94, (1, 1, 0): 87, (1, 2, 1): 107, (1, 2, 0): 100, (1, 4, 1): 132, (1, 4, 0): 132,
    (2, 1, 1): 143, (2, 1, 0): 141, (2, 2, 1): 143, (2, 2, 0): 137, (2, 4, 1): 156, (2, 4, 0): 156,
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
        m = re.search(r"\s(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_predict_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_predict.hip")
    assert got, "no resource remarks from hipcc for bsc_predict.hip"
    kernels = {k: v for k, v in got.items() if "predict_kernel" in k}
    assert len(kernels) == len(MEASURED), sorted(kernels)
    for (fam, nc, full), vgprs in MEASURED.items():
        needle = "predict_kernelILi%dELi%dELb%dE" % (fam, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_predict.hip (renamed?)" % needle
        for name, r in matches.items():
            print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD, %d bytes of LDS" % (
                name, r["VGPRs"], r["ScratchSize"], r["Occupancy"], r["LDS"]))
            assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
            assert r["VGPRs"] <= vgprs + HEADROOM, "%s: %d VGPRs > %d" % (name, r["VGPRs"], vgprs + HEADROOM)
            assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])
    finish = [v for k, v in got.items() if "predict_sum_kernel" in k]
    assert len(finish) == 1 and finish[0]["ScratchSize"] == 0
