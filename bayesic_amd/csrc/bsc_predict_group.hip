// The predictive pass of the random-intercept model (csrc/bsc_glm_group.hip, svi/hier_glm.py): csrc/bsc_predict_pass.h's
// body with OFFS and GRP on, for the logistic and the Poisson family,
//     l_ns = x_n . w_s + b_s[g_n] + o_n.
// The intercept draws come as a table Bt [J + 1][ldb] with the draws contiguous (Bt[j][s] = b_s[j]), so the four draws a
// lane needs of each accumulator chunk are ONE 16-byte buffer load; row J holds the draws of a group that was not seen
// in training (id -1).  The table is 4 (J + 1) ldb bytes -- 256 KB at J = 1000, S = 64 -- and stays in the L2 / MALL
// while X streams past it.  A tile's ids ride with its y and offset; its intercepts are requested at the top of its
// first strip and are covered by the strips' MFMAs (csrc/bsc_predict_pass.h).  The descriptor of the gather covers the
// table exactly, so no id can read outside it; ids are range-CHECKED by bsc_group_ids_check, once per batch, which is
// the second entry point here.  A translation unit of its own so that the shipped predictive kernels keep their names
// and their code.
#include "bsc_predict_pass.h"

namespace {

// FULL: D == 256.  offset may be null.
template <int FAM, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_group_kernel(PredictArgs a, const float* __restrict__ offset,
                                                                   PredictGroups gr) {
    predict_body<PredictFamily<FAM>, NC, FULL, /*OFFS=*/true, /*GRP=*/true>(a, offset, gr);
}

__global__ __launch_bounds__(BSC_WAVE) void predict_group_sum_kernel(const double* __restrict__ partial, int n,
                                                                     double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int FAM, int NC>
void launch_group_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const PredictGroups& gr, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS)
        hipLaunchKernelGGL((predict_group_kernel<FAM, NC, true>), grid, block, 0, ctx->stream, a, offset, gr);
    else
        hipLaunchKernelGGL((predict_group_kernel<FAM, NC, false>), grid, block, 0, ctx->stream, a, offset, gr);
}

template <int FAM>
void launch_group(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const PredictGroups& gr, int n_blocks) {
    predict_launch_chunks(a.S, [&](auto nc) { launch_group_nc<FAM, decltype(nc)::value>(ctx, a, offset, gr, n_blocks); });
}

// ---- the range check of a batch's ids -----------------------------------------------------------------------------------

constexpr int IDS_BLOCK = 256;
constexpr int IDS_MAX_BLOCKS = 1024;
constexpr unsigned long long IDS_NONE = ~0ull;

// *first = the smallest row whose id is outside [lo, J) (an integer minimum: the same answer in any order).
__global__ __launch_bounds__(IDS_BLOCK) void group_ids_check_kernel(const int32_t* __restrict__ g, int64_t B, int lo,
                                                                    int J, unsigned long long* __restrict__ first) {
    unsigned long long mine = IDS_NONE;
    for (int64_t n = (int64_t)blockIdx.x * IDS_BLOCK + threadIdx.x; n < B; n += (int64_t)gridDim.x * IDS_BLOCK) {
        const int id = g[n];
        if ((id < lo || id >= J) && mine == IDS_NONE) mine = (unsigned long long)n;
    }
    if (mine != IDS_NONE) atomicMin(first, mine);
}

}  // namespace

extern "C" {

int bsc_predict_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                            const float* offset, const int32_t* groups, int64_t B, int32_t D, int32_t J, const float* W,
                            const float* Bt, int32_t ldb, int32_t S, float* mean, float* var, float* lpd,
                            double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_predict_pass_groups";
    PREDICT_UNSUPPORTED(family == BSC_PREDICT_LOGISTIC || family == BSC_PREDICT_POISSON,
                        "%s: family=%d must be BSC_PREDICT_LOGISTIC (1) or BSC_PREDICT_POISSON (2): the random-intercept "
                        "model has these two links", who, family);
    int rc = predict_check_batch(who, X, y, B, W, mean, var, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    rc = predict_check_groups(who, groups, Bt, J, ldb, S);
    if (rc != BSC_OK) return rc;
    PREDICT_UNSUPPORTED((((uintptr_t)groups) & 3) == 0 && (((uintptr_t)offset) & 3) == 0,
                        "%s: groups and offset must be 4-byte aligned", who);
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, y, B, D, W, nullptr, S, mean, var, lpd, lpd_sum, &a, &n_blocks);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    PredictGroups gr;
    gr.g = groups; gr.Bt = Bt; gr.J = J; gr.ldb = ldb;
    {
        bsc_prof_scope prof(ctx);
        if (family == BSC_PREDICT_LOGISTIC) launch_group<BSC_PREDICT_LOGISTIC>(ctx, a, offset, gr, n_blocks);
        else launch_group<BSC_PREDICT_POISSON>(ctx, a, offset, gr, n_blocks);
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(predict_group_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream, (const double*)a.partial,
                           n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

int bsc_group_ids_check(bsc_ctx* ctx, const int32_t* groups, int64_t B, int32_t J, int32_t allow_new) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_group_ids_check";
    BSC_REQUIRE(!ctx->capturing, "%s inside a graph capture", who);
    BSC_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE(groups || B == 0, "%s: groups is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)groups) & 3) == 0, "%s: groups must be 4-byte aligned", who);
    if (B == 0) return BSC_OK;
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, sizeof(unsigned long long), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;   // pass partials that were pending in the workspace are gone
    unsigned long long* first = (unsigned long long*)ws;
    BSC_HIP(hipMemsetAsync(first, 0xFF, sizeof(unsigned long long), ctx->stream));
    const int64_t want = (B + IDS_BLOCK - 1) / IDS_BLOCK;
    const int n_blocks = (int)(want < IDS_MAX_BLOCKS ? want : IDS_MAX_BLOCKS);
    hipLaunchKernelGGL(group_ids_check_kernel, dim3(n_blocks), dim3(IDS_BLOCK), 0, ctx->stream, groups, B,
                       allow_new ? -1 : 0, (int)J, first);
    BSC_LAUNCH_CHECK();
    unsigned long long row = IDS_NONE;
    BSC_HIP(hipMemcpyAsync(&row, first, sizeof(row), hipMemcpyDeviceToHost, ctx->stream));
    BSC_HIP(hipStreamSynchronize(ctx->stream));
    if (row == IDS_NONE) return BSC_OK;
    int32_t id = 0;
    BSC_HIP(hipMemcpy(&id, groups + row, sizeof(id), hipMemcpyDeviceToHost));
    if (allow_new) return bsc_fail(BSC_ERR_INVALID, "%s: row %lld has group id %d outside [-1,%d)", who, (long long)row, id, J);
    return bsc_fail(BSC_ERR_INVALID, "%s: row %lld has group id %d outside [0,%d)", who, (long long)row, id, J);
}

}  // extern "C"
