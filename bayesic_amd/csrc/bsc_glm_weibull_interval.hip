// Interval and left censoring for the Weibull survival route (csrc/bsc_glm_weibull.hip): csrc/bsc_glm_pass.h's bodies with
// the per-draw scalar flag AND the upper-end flag on, their slab reduction, and csrc/bsc_predict_pass.h's body with the
// interval variant of its sixth family.  The finishes (bsc_glm_weibull_update, bsc_glm_scalar_fullrank_update) see
// [ell | G | T] alone and are shared as they are.
//
// One more per-row vector, upper [B] float32, next to the signed y of csrc/bsc_glm_weibull.hip:
//     upper[n] == 0             the row is what y[n] says: y > 0 an event at y, y < 0 right-censored at -y
//     upper[n] >  0, y[n] < 0   interval-censored: the event lies in (a, b] = (-y[n], upper[n]],  b > a
//     upper[n] <  0             left-censored: the event is at or before b = -upper[n]; the magnitude of y[n] is not read
// so a vector of zeros (and the rows past B, which read 0 through the descriptor) is today's model.  With la = log a,
// d = log b - la > 0, z_a = k (la - l), E_a = e^{z_a}, Delta = E_a expm1(k d) = E_b - E_a (a narrow interval does not
// cancel) and E_b = E_a + Delta, an interval row adds
//     log P  = -E_a + log(-expm1(-Delta))                                  (= log(S(a) - S(b)): nothing left out)
//     d / dl   = k ( E_a - Delta / expm1(Delta) )
//     d / dtau = -z_a E_a + ( z_a Delta + k d E_b ) / expm1(Delta)
// and a left-censored row the same with E_a = 0, z_a E_a = 0, Delta = E_b:  log P = log(-expm1(-E_b)),
// d / dl = -k E_b / expm1(E_b),  d / dtau = z_b E_b / expm1(E_b).  Where Delta >= 103 (e^{-Delta} is zero in float32), or
// e^{k d} is infinite in float32 (upper = 1e30 for "no bound"), the row is the right-censored one at a -- a left-censored
// one adds nothing -- by selects on the link's inputs (glm_link).  Apart from that the link is NOT clamped: finite while
// z_a stays below about 88.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_glm_pass.h"
#include "bsc_predict_pass.h"

namespace {

constexpr int MAX_S = 64;

// ---- the pass ---------------------------------------------------------------------------------------------------------

template <bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_weibull_itv_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, const float* __restrict__ u, int64_t B, int D, const float* __restrict__ W,
    const float* __restrict__ logshape, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_body<GLM_WEIBULL, FULL, true, false, true, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr,
                                                              logshape, u);
}

__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_weibull_itv_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, const float* __restrict__ u, int64_t B, const float* __restrict__ W,
    const float* __restrict__ logshape, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GLM_WEIBULL, true, false, true, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logshape,
                                                             u);
}

__global__ __launch_bounds__(RED_BLOCK) void glm_weibull_itv_slab_reduce_kernel(const float* __restrict__ slab,
                                                                                int n_blocks, int D, int S, int s_base,
                                                                                double* __restrict__ ell,
                                                                                double* __restrict__ G,
                                                                                double* __restrict__ T) {
    regress_slab_reduce<NB_SLAB_STRIDE>(slab, n_blocks, D, S, s_base, ell, G, T);
}

// dsp_data_pass (csrc/bsc_glm_pass.h) with the upper ends: the same envelope, grid, slab and chunks of eight draws; `upper`
// (not null) joins the vectors whose alignment decides the MFMA route and is handed to the kernels behind the weight.
int itv_data_pass(bsc_ctx* ctx, const char* who, const float* X, int64_t ldx, const float* y, const float* upper,
                  const float* offset, const float* weight, int64_t B, int32_t D, const float* W, const float* logshape,
                  int32_t S, double* ell, double* G, double* T) {
    const int rc0 = check_glm_obs_args(who, BSC_GLM_LOGISTIC, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc0 != BSC_OK) return rc0;
    BSC_REQUIRE((((uintptr_t)upper) & 3) == 0, "%s: upper must be 4-byte aligned", who);
    BSC_REQUIRE(logshape, "%s: logshape is null", who);
    BSC_REQUIRE((((uintptr_t)logshape) & 3) == 0, "%s: logshape must be 4-byte aligned", who);
    BSC_REQUIRE(ell && G && T, "%s: null output", who);

    const int rows = pass_rows(D, y, offset, weight, nullptr, upper);
    const PassGrid g = pass_grid(ctx, B, rows);
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * NB_SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    const dim3 rgrid((NB_SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, offset, weight, upper,
                           B, tail...);
    };
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {   // each launch with its chunk of the shape draws
            const float *Ws = W + (int64_t)s0 * D, *lp = logshape + s0;
            launch_pass_shape(rows, D, [&] { go(glm_weibull_itv_pass_mfma_kernel, Ws, lp, sg, slab, g.n_iter); },
                              [&](auto full) {
                                  go(glm_weibull_itv_pass_kernel<decltype(full)::value>, (int)D, Ws, lp, sg, slab,
                                     g.n_iter);
                              });
        },
        [&](int s0) {
            hipLaunchKernelGGL(glm_weibull_itv_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream,
                               (const float*)slab, g.n_blocks, (int)D, (int)S, s0, ell, G, T);
        });
}

// ---- the predictive ---------------------------------------------------------------------------------------------------

// FULL: D == 256.  offset may be null, upper is set.
template <int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_weibull_itv_kernel(PredictArgs a, const float* __restrict__ offset,
                                                                         const float* __restrict__ upper) {
    predict_body<PREDICT_WEIBULL, NC, FULL, true, false, true>(a, offset, PredictGroups{}, upper);
}

__global__ __launch_bounds__(BSC_WAVE) void predict_weibull_itv_sum_kernel(const double* __restrict__ partial, int n,
                                                                           double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int NC>
void launch_predict_weibull_itv_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const float* upper,
                                   int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS)
        hipLaunchKernelGGL((predict_weibull_itv_kernel<NC, true>), grid, block, 0, ctx->stream, a, offset, upper);
    else
        hipLaunchKernelGGL((predict_weibull_itv_kernel<NC, false>), grid, block, 0, ctx->stream, a, offset, upper);
}

}  // namespace

extern "C" {

int bsc_glm_weibull_data_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                       const float* offset, const float* weight, int64_t B, int32_t D, const float* W,
                                       const float* logshape, int32_t S, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    if (!upper)   // the kernels of csrc/bsc_glm_weibull.hip: the same bits
        return bsc_glm_weibull_data_pass(ctx, X, ldx, y, offset, weight, B, D, W, logshape, S, ell, G, T);
    return itv_data_pass(ctx, "bsc_glm_weibull_data_pass_interval", X, ldx, y, upper, offset, weight, B, D, W, logshape,
                         S, ell, G, T);
}

int bsc_weibull_predict_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                      const float* offset, int64_t B, int32_t D, const float* W, const float* logshape,
                                      int32_t S, float* mean, float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    if (!upper) return bsc_weibull_predict_pass(ctx, X, ldx, y, offset, B, D, W, logshape, S, mean, var, lpd, lpd_sum);
    BSC_REQUIRE((((uintptr_t)upper) & 3) == 0, "bsc_weibull_predict_pass_interval: upper must be 4-byte aligned");
    return scalar_predict_pass(
        ctx, "bsc_weibull_predict_pass_interval", "logshape",
        [&](auto nc, const PredictArgs& a, int n_blocks) {
            launch_predict_weibull_itv_nc<decltype(nc)::value>(ctx, a, offset, upper, n_blocks);
        },
        predict_weibull_itv_sum_kernel, X, ldx, y, offset, B, D, W, logshape, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
