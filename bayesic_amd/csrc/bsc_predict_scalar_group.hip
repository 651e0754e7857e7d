// The predictive pass of the random-intercept models with a learned scalar (csrc/bsc_glm_scalar_group.hip,
// svi/hier_scalar.py): csrc/bsc_predict_pass.h's body with OFFS and GRP on for the negative-binomial, the Gamma and the
// Weibull family,
//     l_ns = x_n . w_s + b_s[g_n] + o_n,      log p(y_n | l_ns, e^{tau_s}) the family's.
// The intercept table Bt [J + 1][ldb], its gather and its descriptor are csrc/bsc_predict_group.hip's; the per-draw
// scalar and its constants ride in the LDS as in csrc/bsc_scalar_family.h's predictive.  Ids are range-CHECKED by
// bsc_group_ids_check, once per batch.  A translation unit of its own so that the shipped predictive kernels keep their
// names and their code.
#include "bsc_predict_pass.h"

namespace {

// FULL: D == 256.  offset may be null.
template <int FAM, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void scalar_predict_group_kernel(PredictArgs a,
                                                                          const float* __restrict__ offset,
                                                                          PredictGroups gr) {
    predict_body<PredictFamily<FAM>, NC, FULL, /*OFFS=*/true, /*GRP=*/true>(a, offset, gr);
}

__global__ __launch_bounds__(BSC_WAVE) void scalar_predict_group_sum_kernel(const double* __restrict__ partial, int n,
                                                                            double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int FAM, int NC>
void launch_group_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const PredictGroups& gr, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS)
        hipLaunchKernelGGL((scalar_predict_group_kernel<FAM, NC, true>), grid, block, 0, ctx->stream, a, offset, gr);
    else
        hipLaunchKernelGGL((scalar_predict_group_kernel<FAM, NC, false>), grid, block, 0, ctx->stream, a, offset, gr);
}

template <int FAM>
void launch_group(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const PredictGroups& gr, int n_blocks) {
    predict_launch_chunks(a.S,
                          [&](auto nc) { launch_group_nc<FAM, decltype(nc)::value>(ctx, a, offset, gr, n_blocks); });
}

}  // namespace

extern "C" {

int bsc_scalar_predict_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                                   const float* offset, const int32_t* groups, int64_t B, int32_t D, int32_t J,
                                   const float* W, const float* Bt, int32_t ldb, const float* logtau, int32_t S,
                                   float* mean, float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_scalar_predict_pass_groups";
    PREDICT_UNSUPPORTED(scalar_family_ok(family),
                        "%s: family=%d must be BSC_SCALAR_NEGBIN (0), BSC_SCALAR_GAMMA (1) or BSC_SCALAR_WEIBULL (2)",
                        who, family);
    int rc = predict_check_batch(who, X, y, B, W, mean, var, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(logtau, "%s: logtau is null", who);
    rc = predict_check_groups(who, groups, Bt, J, ldb, S);
    if (rc != BSC_OK) return rc;
    PREDICT_UNSUPPORTED((((uintptr_t)groups) & 3) == 0 && (((uintptr_t)offset) & 3) == 0 &&
                            (((uintptr_t)logtau) & 3) == 0,
                        "%s: groups, offset and logtau must be 4-byte aligned", who);
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, y, B, D, W, logtau, S, mean, var, lpd, lpd_sum, &a, &n_blocks);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    PredictGroups gr;
    gr.g = groups; gr.Bt = Bt; gr.J = J; gr.ldb = ldb;
    {
        bsc_prof_scope prof(ctx);
        with_scalar_family(family,
                           [&](auto f) { launch_group<decltype(f)::PREDICT_ID>(ctx, a, offset, gr, n_blocks); });
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(scalar_predict_group_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream,
                           (const double*)a.partial, n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
