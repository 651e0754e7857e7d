// The per-group sums of the grouped passes' residuals (csrc/bsc_glm_group.hip's header comment describes them): the
// plan layout of bsc_glm_group_plan and the two kernels that sum R through it, without float atomics and in an order that
// depends on the plan alone.  Shared by csrc/bsc_glm_group.hip (logistic, Poisson) and csrc/bsc_glm_scalar_group.hip
// (the families with a learned scalar); each translation unit gets its own glm_group_segment_kernel and
// glm_group_sum_kernel.  Header-only, internal linkage, like csrc/bsc_regress.h.
#pragma once

#include "bsc_glm_pass.h"

namespace {

constexpr int SEG_ROWS = BSC_GLM_GROUP_SEG_ROWS;
constexpr int PLAN_HDR = 8;               // [magic, B, J, n_seg, SEG_ROWS, 0, 0, 0]
constexpr int32_t PLAN_MAGIC = 0x67726f75;

// The plan, int32: header | perm [B] | first segment of group j [J + 1] | (start, length, group) per segment.
// Every offset follows from (B, J), which the caller of the pass passes again: the kernels never trust the header for
// an address, they only refuse a plan whose header names another batch.
inline int64_t plan_perm_off() { return PLAN_HDR; }
__host__ __device__ inline int64_t plan_grp_off(int64_t B) { return PLAN_HDR + B; }
__host__ __device__ inline int64_t plan_seg_off(int64_t B, int J) { return PLAN_HDR + B + J + 1; }
inline int64_t plan_seg_bound(int64_t B, int J) {   // sum_j ceil(c_j / SEG_ROWS) <= B / SEG_ROWS + min(J, B)
    return B / SEG_ROWS + (B < J ? B : (int64_t)J);
}

__device__ __forceinline__ bool plan_matches(const int32_t* __restrict__ plan, int64_t B, int J) {
    return plan[0] == PLAN_MAGIC && (int64_t)plan[1] == B && plan[2] == J && plan[4] == SEG_ROWS;
}

// One wave per segment: lane = (row-lane lane >> 3, draw lane & 7).  segsum[seg][draw], float64.
constexpr int SEG_BLOCK = 256;
__global__ __launch_bounds__(SEG_BLOCK) void glm_group_segment_kernel(const int32_t* __restrict__ plan, int64_t B,
                                                                      int J, int64_t seg_bound,
                                                                      const float* __restrict__ R,
                                                                      double* __restrict__ segsum) {
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * (SEG_BLOCK / BSC_WAVE) + (threadIdx.x >> 6);
    if (!plan_matches(plan, B, J)) return;
    int64_t n_seg = plan[3];
    if (n_seg > seg_bound) n_seg = seg_bound;
    if (seg >= n_seg) return;
    const int32_t* __restrict__ perm = plan + PLAN_HDR;
    const int32_t* __restrict__ tab = plan + plan_seg_off(B, J) + 3 * seg;
    int64_t start = tab[0], len = tab[1];
    if (start < 0 || len < 0 || len > SEG_ROWS || start + len > B) len = 0;   // not a plan of bsc_glm_group_plan
    const int rl = lane >> 3, s = lane & 7;
    double acc = 0.0;
    for (int i0 = rl; i0 < len; i0 += 32) {      // four rows in flight per lane, added in row order
        float r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 8 * u;
            r[u] = 0.f;
            if (i < len) {
                const int64_t row = perm[start + i];
                if (row >= 0 && row < B) r[u] = R[(row >> 4) * R_BLOCK + s * 16 + (row & 15)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += (double)r[u];
    }
    acc += __shfl_xor(acc, 8);
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    if (lane < 8) segsum[seg * SG + s] = acc;
}

// H[s_base + s][j] = the segments of group j in segment order; thread = (group, draw slot).
__global__ __launch_bounds__(256) void glm_group_sum_kernel(const int32_t* __restrict__ plan, int64_t B, int J,
                                                            int64_t seg_bound, const double* __restrict__ segsum,
                                                            int S, int s_base, double* __restrict__ H) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int j = idx >> 3, s = idx & 7;
    if (j >= J || s_base + s >= S) return;
    double tot = 0.0;
    if (!plan_matches(plan, B, J)) {
        tot = __builtin_nan("");     // a plan built for another batch: loud, and nothing was read through it
    } else {
        const int32_t* __restrict__ grp = plan + plan_grp_off(B);
        int64_t first = grp[j], last = grp[j + 1];
        if (first < 0) first = 0;
        if (last > seg_bound) last = seg_bound;
        for (int64_t k = first; k < last; ++k) tot += segsum[k * SG + s];
    }
    H[(int64_t)(s_base + s) * J + j] = tot;
}

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }

// The launches of a chunk's group sums on ctx's stream: R -> segsum -> H[s_base ..].
inline int launch_group_sums(bsc_ctx* ctx, const int32_t* plan, int64_t B, int J, int64_t seg_bound, const float* R,
                             double* segsum, int S, int s_base, double* H) {
    const unsigned seg_grid = (unsigned)((seg_bound + SEG_BLOCK / BSC_WAVE - 1) / (SEG_BLOCK / BSC_WAVE));
    const unsigned sum_grid = (unsigned)(((int64_t)J * SG + 255) / 256);
    if (seg_grid) {
        hipLaunchKernelGGL(glm_group_segment_kernel, dim3(seg_grid), dim3(SEG_BLOCK), 0, ctx->stream, plan, B, J,
                           seg_bound, R, segsum);
        BSC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(glm_group_sum_kernel, dim3(sum_grid), dim3(256), 0, ctx->stream, plan, B, J, seg_bound,
                       (const double*)segsum, S, s_base, H);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // namespace
