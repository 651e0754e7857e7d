// The predictive pass with a per-row offset: csrc/bsc_predict_pass.h's body with OFFS on, for the logistic and the
// Poisson family (l_ns = x_n . w_s + o_n; the Gaussian family takes no offset).  A translation unit of its own so
// that predict_kernel of csrc/bsc_predict.hip keeps its name and its code; the entry point (bsc_predict_pass_offset)
// is in that file.
#include "bsc_predict_pass.h"

namespace {

template <int FAM, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_offset_kernel(PredictArgs a, const float* __restrict__ offset) {
    predict_body<PredictFamily<FAM>, NC, FULL, true>(a, offset);
}

template <int FAM, int NC>
void launch_offset_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS) hipLaunchKernelGGL((predict_offset_kernel<FAM, NC, true>), grid, block, 0, ctx->stream, a, offset);
    else hipLaunchKernelGGL((predict_offset_kernel<FAM, NC, false>), grid, block, 0, ctx->stream, a, offset);
}

template <int FAM>
void launch_offset(bsc_ctx* ctx, const PredictArgs& a, const float* offset, int n_blocks) {
    predict_launch_chunks(a.S, [&](auto nc) { launch_offset_nc<FAM, decltype(nc)::value>(ctx, a, offset, n_blocks); });
}

}  // namespace

void bsc_predict_offset_launch(bsc_ctx* ctx, int family, const void* predict_args, const float* offset, int n_blocks) {
    const PredictArgs& a = *static_cast<const PredictArgs*>(predict_args);
    if (family == BSC_PREDICT_LOGISTIC) launch_offset<BSC_PREDICT_LOGISTIC>(ctx, a, offset, n_blocks);
    else launch_offset<BSC_PREDICT_POISSON>(ctx, a, offset, n_blocks);
}
