// The GLM training pass with per-row offsets and weights: csrc/bsc_glm_pass.h's bodies with OBS on.
//
//     l[n,s] = x_n . w_s + o[n]
//     ell[s] = sum_n v[n] (y[n] l[n,s] - A(l[n,s]))           G[s, :] = sum_n v[n] (y[n] - A'(l[n,s])) x_n
//
// An offset is how a rate model carries its exposure (log E[y_n] = x_n . w + log exposure_n); weights are aggregated
// binomial rows, survey weights and row masks.  Eight more bytes per row next to the 4 D + 4 the pass streams, so the
// two vectors ride in the pass's own tiles: the kernels are csrc/bsc_glm.hip's, one instantiation per (tile shape,
// link) -- a null offset reads 0 through an empty descriptor, a null weight is a uniform select of 1.0f.  They live in
// a translation unit of their own so that the kernels of csrc/bsc_glm.hip keep their names and their code; the entry
// points (bsc_glm_data_pass_obs, bsc_glm_pass_update_obs) are in that file, next to the slab and the finish they share.
#include "bsc_glm_pass.h"

namespace {

template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_obs_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, int S, float* __restrict__ slab,
    int n_iter) {
    glm_pass_body<GlmFamily<LINK>, FULL, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_obs_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, int S, float* __restrict__ slab,
    int n_iter) {
    glm_pass_mfma_body<GlmFamily<LINK>, true>(X, ldx, y, o, v, B, W, S, slab, n_iter);
}

template <int LINK>
void launch_obs_link(bsc_ctx* ctx, int mfma, const float* X, int64_t ldx, const float* y, const float* o,
                     const float* v, int64_t B, int D, const float* W, int sg, int n_blocks, int n_iter, float* slab) {
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, o, v, B, tail...);
    };
    launch_pass_shape(mfma ? MT_ROWS : ROWS, D, [&] { go(glm_obs_pass_mfma_kernel<LINK>, W, sg, slab, n_iter); },
                      [&](auto full) { go(glm_obs_pass_kernel<LINK, decltype(full)::value>, D, W, sg, slab, n_iter); });
}

}  // namespace

void bsc_glm_obs_launch_pass(bsc_ctx* ctx, int link, int mfma, const float* X, int64_t ldx, const float* y,
                             const float* offset, const float* weight, int64_t B, int D, const float* W, int sg,
                             int n_blocks, int n_iter, float* slab) {
    if (link == BSC_GLM_LOGISTIC)
        launch_obs_link<BSC_GLM_LOGISTIC>(ctx, mfma, X, ldx, y, offset, weight, B, D, W, sg, n_blocks, n_iter, slab);
    else
        launch_obs_link<BSC_GLM_POISSON>(ctx, mfma, X, ldx, y, offset, weight, B, D, W, sg, n_blocks, n_iter, slab);
}
