"""Compile-time resource guard for the GLM pass kernels with offsets and weights (csrc/bsc_glm_obs.hip) and the
predictive pass with an offset (csrc/bsc_predict_offset.hip), as tests/test_glm_kernel_resources.py and
tests/test_predict_kernel_resources.py keep for the kernels without them (no GPU needed: hipcc cross-compiles for
gfx950; only the compiler's resource remarks are read).

Measured from this compile (VGPRs, scratch bytes per lane, waves per SIMD):

    glm_obs_pass_mfma_kernel<logistic>          214, 0, 2        glm_obs_pass_mfma_kernel<poisson>          212, 0, 2
    glm_obs_pass_kernel<logistic, D == 256>     221, 0, 2        glm_obs_pass_kernel<poisson, D == 256>     219, 0, 2
    glm_obs_pass_kernel<logistic, D < 256>      223, 0, 2        glm_obs_pass_kernel<poisson, D < 256>      220, 0, 2

(the kernels without offset and weight: 200 / 198, 216 / 216, 221 / 216).  The pass kernels are launched for two waves
per SIMD: 256 VGPRs at most; the guard is the measured count plus 24, capped at 256.

predict_offset_kernel<family, chunks of 16 draws, D == 256> (VGPRs; scratch 0 and 2 waves per SIMD for every one):

    family     chunks 1: D == 256, other     chunks 2: D == 256, other     chunks 4: D == 256, other
    logistic             96         88                 108       101                 133       133
    poisson             145        141                 145       137                 157       157
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADROOM = 24

# mangled-name substring -> VGPRs as measured
PASS_KERNELS = {
    "glm_obs_pass_mfma_kernelILi0E": 214,
    "glm_obs_pass_mfma_kernelILi1E": 212,
    "glm_obs_pass_kernelILi0ELb1E": 221,
    "glm_obs_pass_kernelILi0ELb0E": 223,
    "glm_obs_pass_kernelILi1ELb1E": 219,
    "glm_obs_pass_kernelILi1ELb0E": 220,
}

# (family, chunks, D == 256) -> VGPRs as measured
PREDICT_KERNELS = {
    (1, 1, 1): 96, (1, 1, 0): 88, (1, 2, 1): 108, (1, 2, 0): 101, (1, 4, 1): 133, (1, 4, 0): 133,
    (2, 1, 1): 145, (2, 1, 0): 141, (2, 2, 1): 145, (2, 2, 0): 137, (2, 4, 1): 157, (2, 4, 0): 157,
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


def _check(name, r, measured):
    limit = min(measured + HEADROOM, 256)
    print("%s: %d VGPRs, %d bytes of scratch, %d waves/SIMD" % (name, r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
    assert r["ScratchSize"] == 0, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
    assert r["VGPRs"] <= limit, "%s: %d VGPRs > %d" % (name, r["VGPRs"], limit)
    assert r["Occupancy"] >= 2, "%s: %d waves per SIMD" % (name, r["Occupancy"])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_glm_obs_pass_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_glm_obs.hip")
    assert got, "no resource remarks from hipcc for bsc_glm_obs.hip"
    assert len([k for k in got if "pass" in k and "kernel" in k]) == len(PASS_KERNELS), sorted(got)
    for needle, measured in PASS_KERNELS.items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_glm_obs.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_predict_offset_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    got = resources("bsc_predict_offset.hip")
    assert got, "no resource remarks from hipcc for bsc_predict_offset.hip"
    kernels = {k: v for k, v in got.items() if "predict_offset_kernel" in k}
    assert len(kernels) == len(PREDICT_KERNELS), sorted(kernels)
    for (fam, nc, full), measured in PREDICT_KERNELS.items():
        needle = "predict_offset_kernelILi%dELi%dELb%dE" % (fam, nc, full)
        matches = {k: v for k, v in kernels.items() if needle in k}
        assert len(matches) == 1, "kernel %s not found in bsc_predict_offset.hip (renamed?)" % needle
        for name, r in matches.items():
            _check(name, r, measured)
            assert r["LDS"] <= 160 * 1024, "%s: %d bytes of LDS" % (name, r["LDS"])
