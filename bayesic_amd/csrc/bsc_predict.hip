// Posterior predictive and held-out log density for the regression models of csrc/bsc_blr.hip and csrc/bsc_glm.hip.
//
// ABSENT in the reference (it has no inference code, so nothing to predict from).  With l_ns = x_n . w_s for S draws
// of the fitted q, per row n:
//     mean_n = 1/S sum_s mu(l_ns)
//     var_n  = 1/S sum_s v(l_ns) + 1/S sum_s (mu(l_ns) - mean_n)^2                (law of total variance)
//     lpd_n  = logsumexp_s log p(y_n | l_ns) - log S
// and lpd_sum = sum_n lpd_n in float64.  Only the forward contraction of the training passes, reduced over DRAWS
// within a row instead of over rows: no backward half, no slab, so nothing fills the register file and ONE read of
// X serves every S <= 64 (the training passes re-read X once per eight draws).
//
// predict_kernel: 512 threads = 8 waves = two per SIMD, one workgroup per CU (LDS-limited: 16 * ceil16(S) / 16
// KiB of W + 65 KiB of tiles of the 160 KiB).  W[S, D] is staged once per workgroup, zero-padded to
// [16 NC][258] (NC = 1, 2, 4 chunks of 16 draws).  A wave owns 16-row tiles; a tile crosses the LDS in two strips of 128 columns
// (a whole tile per wave next to 64 KiB of W would not fit), each prefetched through registers by non-temporal
// 16-byte buffer loads (two rows of 512 contiguous bytes per instruction) while the strip before it is contracted.
// The contraction runs on v_mfma_f32_16x16x4_f32 for every S with W as the A operand and the tile as B: lane
// (i16 = lane % 16, kq = lane / 16) supplies W[16 c + i16][k] and X[row i16][k], k = 128 h + kw kq + 2 j + e, both
// by 8-byte LDS reads (row strides 258 and 130 floats = 2 mod 64: the 32 lanes of a read hit 32 different bank
// pairs), and ends with l(row i16, draw 16 c + 4 kq + reg) in register reg of accumulator c.  So a row's draws sit
// in four lanes x 4 NC registers, all at once: the moments are the two-pass ones (sum -> mean, then squares about
// that mean; never E[mu^2] - E[mu]^2), the log-mean-exp subtracts the maximum over all draws, the lane folds are
// two butterflies over lane bits 4 and 5, and lanes 0 .. 15 store one row each.
// Rows past the end read as zeros through the buffer descriptors and are not stored.
// lpd_sum: float64 lane sums in tile order -> wave -> block partial in wave order -> one fixed-order finish.  No
// float atomics: bitwise reproducible.
#include "bsc_predict_pass.h"

namespace {

// FULL: D == 256 (two strips, 32 columns per lane group, everything unrolled).
template <int FAM, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_kernel(PredictArgs a) {
    predict_body<PredictFamily<FAM>, NC, FULL, false>(a, nullptr);
}

// lpd_sum = the block partials in block order
__global__ __launch_bounds__(BSC_WAVE) void predict_sum_kernel(const double* __restrict__ partial, int n,
                                                               double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int FAM, int NC>
void launch_predict_nc(bsc_ctx* ctx, const PredictArgs& a, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS) hipLaunchKernelGGL((predict_kernel<FAM, NC, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((predict_kernel<FAM, NC, false>), grid, block, 0, ctx->stream, a);
}

template <int FAM>
void launch_predict(bsc_ctx* ctx, const PredictArgs& a, int n_blocks) {
    predict_launch_chunks(a.S, [&](auto nc) { launch_predict_nc<FAM, decltype(nc)::value>(ctx, a, n_blocks); });
}

// Both entry points; `offset` is null for bsc_predict_pass.
int predict_impl(bsc_ctx* ctx, const char* who, int32_t family, const float* X, int64_t ldx, const float* y,
                 const float* offset, int64_t B, int32_t D, const float* W, const float* logvar, int32_t S, float* mean,
                 float* var, float* lpd, double* lpd_sum) {
    BSC_REQUIRE(family == BSC_PREDICT_GAUSSIAN || family == BSC_PREDICT_LOGISTIC || family == BSC_PREDICT_POISSON,
                "%s: family=%d must be BSC_PREDICT_GAUSSIAN (0), BSC_PREDICT_LOGISTIC (1) or BSC_PREDICT_POISSON (2)",
                who, family);
    int rc = predict_check_batch(who, X, y, B, W, mean, var, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(family != BSC_PREDICT_GAUSSIAN || logvar, "%s: the Gaussian family needs logvar[S]", who);
    BSC_REQUIRE(family != BSC_PREDICT_GAUSSIAN || !offset,
                "%s: offset is for BSC_PREDICT_LOGISTIC and BSC_PREDICT_POISSON; the Gaussian family takes none", who);
    BSC_REQUIRE((((uintptr_t)offset) & 3) == 0, "%s: offset must be 4-byte aligned", who);
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, y, B, D, W, logvar, S, mean, var, lpd, lpd_sum, &a, &n_blocks);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    {
        bsc_prof_scope prof(ctx);
        if (offset) bsc_predict_offset_launch(ctx, family, &a, offset, n_blocks);
        else if (family == BSC_PREDICT_GAUSSIAN) launch_predict<BSC_PREDICT_GAUSSIAN>(ctx, a, n_blocks);
        else if (family == BSC_PREDICT_LOGISTIC) launch_predict<BSC_PREDICT_LOGISTIC>(ctx, a, n_blocks);
        else launch_predict<BSC_PREDICT_POISSON>(ctx, a, n_blocks);
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(predict_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream, a.partial, n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_predict_pass(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                     const float* W, const float* logvar, int32_t S, float* mean, float* var, float* lpd,
                     double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return predict_impl(ctx, "bsc_predict_pass", family, X, ldx, y, nullptr, B, D, W, logvar, S, mean, var, lpd, lpd_sum);
}

int bsc_predict_pass_offset(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                            const float* offset, int64_t B, int32_t D, const float* W, const float* logvar, int32_t S,
                            float* mean, float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return predict_impl(ctx, "bsc_predict_pass_offset", family, X, ldx, y, offset, B, D, W, logvar, S, mean, var, lpd,
                        lpd_sum);
}

}  // extern "C"
