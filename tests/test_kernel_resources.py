"""Compile-time resource guard for the hot kernels (no GPU needed: hipcc cross-compiles).

A streaming kernel that silently picks up scratch or doubles its VGPR count still passes
every parity test and only shows up as a slower benchmark -- this happened once in round 1
(lgamma inlined into every fused map kernel: 62 -> 200 VGPRs + scratch, 3x slower).  The
limits below are what the current code needs plus headroom, and the occupancy each kernel
was tuned for."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel-name substring -> (max VGPRs, max scratch bytes per lane)
LIMITS = {
    "bsc_blr.hip": {
        "blr_pass_q_kernelILb1ELi0ELi1E": (224, 0),     # the default pass: both contractions on v_mfma_f32_4x4x1 (2 waves/SIMD needs <= 256)
        "blr_pass_mx_kernelILb1ELi4E": (256, 0),        # sixteen draws per pass: 64 accumulator registers
        "blr_pass_kernelILb1ELi8ELb1E": (256, 0),
        "blr_fused_update_kernelILi1024E": (128, 0),    # the default: sixteen waves = four per SIMD
        "blr_fused_update_kernelILi512E": (192, 0),     # (A/B variants: eight / four waves, the slab in one trip of
        "blr_fused_update_kernelILi256E": (192, 0),     #  32 loads per lane)
    },
    "bsc_rowsoftmax.hip": {
        "gemm_softmax_rows_kernelILi20E": (256, 0),     # K = 40 (the derived mixture): 2 waves/SIMD, no scratch
        "gemm_softmax_rows_kernelILi8E": (256, 0),
        "gemm_softmax_rows_kernelILi32E": (256, 0),     # K = 64
    },
    "bsc_fused.hip": {
        "map_dense_f32_kernelILi2E": (128, 0),
        "map_reduce_wave_dense_f32_kernelILi2ELi4E": (128, 0),
        "map_reduce_lane_dense_f32_kernelILi2E": (128, 0),
        "map_reduce_lane_narrow_f32_kernelILi3E": (128, 0),
        "map_reduce_wave_kernelIfLb0E": (128, 0),
        "map_strided_kernelIfLb0E": (96, 0),
        "map_flat_f32_kernelILi2ELb1E": (96, 0),
        "map_flat_f32_kernelILi4ELb0E": (128, 0),
        "map_reduce_rows_f32_kernelILi2ELb1E": (128, 0),
    },
    "bsc_lda.hip": {
        "lda_sstats_kernelILi4E": (256, 0),
        "lda_sstats_stream_kernel": (256, 32),       # (spills at the block boundaries, not in a step)
        "lda_sstats_csc_kernelILi8ELb1E": (96, 0),
        # the split-operand route: two workgroups of 80 KiB a CU with two bf16 terms (<= 256 registers, nothing in
        # scratch: a spilled Bt fragment was reloaded in every step once); three terms run one workgroup a CU
        "lda_sstats_bx2_kernel": (240, 0),
        "lda_sstats_bx2_bound_kernel": (240, 0),
        "lda_sstats_bx3_bound_kernel": (384, 0),
    },
    "bsc_gram.hip": {
        "gram256_bx_kernel": (256, 0),                  # eight waves a CU = two per SIMD
    },
    "bsc_gemm.hip": {
        "gemm_f32_mfma_kernelILb1ELb1EE": (256, 0),
        "gemm_f32_mfma_kernelILb0ELb1EE": (256, 0),
        "gemm_f32_dma_kernel": (144, 0),
        # two workgroups per CU: <= 256; the few scratch bytes are spills in the guarded edge-tile
        # store path, outside the k-loop (the loop's own budget is checked in the ISA: DESIGN 12)
        # (100 bytes in the instantiation with operand prologues AND partial tiles, bsc_gemm_fused)
        "gemm_f32_stream_kernel": (256, 112),
    },
    "bsc_skinny.hip": {
        "gemm_skinny_tn_kernel": (128, 0),
        "gemm_skinny_nt_kernelILi2ELi16E": (192, 0),
    },
    "bsc_mog.hip": {
        "mog_estep_kernel": (256, 0),
        "mog_estep_bx_kernel": (256, 8),                # (one register parked before the tile loop and fetched after it)
    },
    "bsc_bbvi.hip": {
        "logreg_loglik_xreg_kernelILb1ELi4E": (160, 0), # X through VGPRs at S = 64 (option bbvi_kernel = 2): three waves/SIMD
        "logreg_loglik_dma_kernelILb1ELi4ELi0E": (192, 0),
        "logreg_loglik_dma_bx_kernel": (200, 0),
        "bbvi_update_kernel": (96, 0),
    },
    "bsc_wouter.hip": {
        # a lambda capturing the prefetch registers once sent them to scratch behind flat
        # loads (3.07 ms instead of 1.77 ms, every parity test green)
        # all KT * CT accumulators live in one wave: two waves per SIMD by design
        "weighted_outer_kernelILi2ELi5E": (256, 0),
        "weighted_outer_kernelILi1ELi8E": (256, 0),
    },
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
        m = re.search(r"\s(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split()[0]] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("source", sorted(LIMITS))
def test_hot_kernels_stay_within_their_register_budget(source):
    got = resources(source)
    assert got, "no resource remarks from hipcc for %s" % source
    for needle, (max_vgpr, max_scratch) in LIMITS[source].items():
        matches = {k: v for k, v in got.items() if needle in k}
        assert matches, "kernel %s not found in %s (renamed?)" % (needle, source)
        for name, r in matches.items():
            assert r["VGPRs"] <= max_vgpr, "%s: %d VGPRs > %d" % (name, r["VGPRs"], max_vgpr)
            assert r["ScratchSize"] <= max_scratch, "%s: %d bytes of scratch" % (name, r["ScratchSize"])
