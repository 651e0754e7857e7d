// The kernels and the host envelopes of the regression families with ONE learned log-scalar behind the weights,
// z = [w (D) | tau]: the negative binomial's dispersion (csrc/bsc_glm_nb.hip), the Gamma shape (csrc/bsc_glm_gamma.hip),
// the Weibull shape (csrc/bsc_glm_weibull.hip), the Weibull route with upper ends (csrc/bsc_glm_weibull_interval.hip),
// the Beta precision (csrc/bsc_glm_beta.hip), the log-normal inverse scale (csrc/bsc_glm_lognormal.hip), the
// zero-inflated Poisson's inflation odds (csrc/bsc_glm_zip.hip) and the Student-t inverse scale
// (csrc/bsc_glm_studentt.hip).
// A family is one struct F of csrc/bsc_families.h -- its two ids (LINK = F::GLM_ID, FAMILY = F::PREDICT_ID), its
// constants and its links -- and the bodies are csrc/bsc_glm_pass.h's, csrc/bsc_predict_pass.h's and
// csrc/bsc_meanfield.h's; what is here is the shell the four units used to repeat:
//
//   kernels   scalar_pass_kernel<LINK, FULL>, scalar_pass_mfma_kernel<LINK>, scalar_slab_reduce_kernel<LINK>,
//             scalar_mf_scalars_kernel<LINK>, scalar_mf_coord_kernel<LINK> (NbModel), scalar_predict_kernel<FAMILY, NC,
//             FULL>, scalar_predict_sum_kernel<FAMILY>; with one more pointer, `upper` [B], behind the weight / the
//             offset: scalar_upper_pass_kernel<LINK, FULL>, scalar_upper_pass_mfma_kernel<LINK>,
//             scalar_upper_predict_kernel<FAMILY, NC, FULL>; with one more float, the family's per-model constant
//             `par` (F::PARAM: the Student-t's degrees of freedom, csrc/bsc_glm_studentt.hip), as the last argument:
//             scalar_par_pass_kernel<LINK, FULL>, scalar_par_pass_mfma_kernel<LINK>, scalar_par_predict_kernel<FAMILY, NC,
//             FULL>.
//   host      scalar_family_data_pass<F, UPPER, PARAM>, scalar_family_update<F>, scalar_family_predict_pass<F, UPPER,
//             PARAM>: the checks, the grid, the workspace and the launches of an entry point, naming their kernels
//             themselves.
//
// A translation unit gets exactly the kernels of the host templates it calls (anonymous namespace, so each unit's are its
// own): a unit that never asks for UPPER has no `upper` kernel and one that never asks for PARAM no `par` kernel, the
// interval unit has no finish.  The next family with a learned scalar is a struct in csrc/bsc_families.h, its id, and
// three extern "C" functions of a few lines.
// Header-only, internal linkage, like csrc/bsc_regress.h.
#pragma once

#include "bsc_glm_pass.h"
#include "bsc_meanfield.h"
#include "bsc_predict_pass.h"

namespace {

constexpr int SCALAR_MAX_S = 64;
static_assert(SCALAR_MAX_S == MF_MAX_S, "the pass and the finish take the same number of draws");

// ---- the pass -------------------------------------------------------------------------------------------------------

template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_body<GlmFamily<LINK>, FULL, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr, logtau);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GlmFamily<LINK>, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logtau);
}

// `u`: the upper ends (csrc/bsc_glm_pass.h, ITV), not null
template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_upper_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, const float* __restrict__ u, int64_t B, int D, const float* __restrict__ W,
    const float* __restrict__ logtau, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_body<GlmFamily<LINK>, FULL, true, false, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr, logtau,
                                                            u);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_upper_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, const float* __restrict__ u, int64_t B, const float* __restrict__ W,
    const float* __restrict__ logtau, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GlmFamily<LINK>, true, false, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logtau,
                                                           u);
}

// `par`: the family's per-model constant (F::PARAM), the same for every draw and every launch of a pass
template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_par_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter, float par) {
    glm_pass_body<GlmFamily<LINK>, FULL, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr, logtau, nullptr,
                                               par);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void scalar_par_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter, float par) {
    glm_pass_mfma_body<GlmFamily<LINK>, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logtau, nullptr, par);
}

template <int LINK>
__global__ __launch_bounds__(RED_BLOCK) void scalar_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                       int D, int S, int s_base,
                                                                       double* __restrict__ ell, double* __restrict__ G,
                                                                       double* __restrict__ T) {
    regress_slab_reduce<NB_SLAB_STRIDE>(slab, n_blocks, D, S, s_base, ell, G, T);
}

// The data pass of an entry point `who`: the 16-row MFMA kernel, the 8-row kernel with D == 256 and with any D, and the
// reduction of the NB_SLAB_STRIDE slab, all S draws in chunks of eight.  `logtau` [S] is the per-draw scalar under the
// name `what`.  UPPER: `upper` (not null) joins the vectors whose alignment decides the MFMA route and is handed to the
// kernels behind the weight; without the flag it is not read.  PARAM: `par`, the family's per-model constant (checked by
// the entry point), is the kernels' last argument; without the flag it is not read.
template <class F, bool UPPER = false, bool PARAM = false>
int scalar_family_data_pass(bsc_ctx* ctx, const char* who, const char* what, const float* X, int64_t ldx,
                            const float* y, const float* upper, const float* offset, const float* weight, int64_t B,
                            int32_t D, const float* W, const float* logtau, int32_t S, double* ell, double* G,
                            double* T, float par = 0.f) {
    constexpr int LINK = F::GLM_ID;
    static_assert(PARAM == F::PARAM && !(UPPER && PARAM), "the constant rides with the family that declares one");
    const int rc0 = check_glm_obs_args(who, BSC_GLM_LOGISTIC, X, ldx, y, offset, weight, B, D, W, S, SCALAR_MAX_S);
    if (rc0 != BSC_OK) return rc0;
    if constexpr (UPPER) BSC_REQUIRE((((uintptr_t)upper) & 3) == 0, "%s: upper must be 4-byte aligned", who);
    BSC_REQUIRE(logtau, "%s: %s is null", who, what);
    BSC_REQUIRE((((uintptr_t)logtau) & 3) == 0, "%s: %s must be 4-byte aligned", who, what);
    BSC_REQUIRE(ell && G && T, "%s: null output", who);

    const int rows = pass_rows(D, y, offset, weight, nullptr, UPPER ? upper : nullptr);
    const PassGrid g = pass_grid(ctx, B, rows);
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * NB_SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    const dim3 rgrid((NB_SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    const auto go = [&](auto kernel, auto... tail) {
        const dim3 grid(g.n_blocks), block(PASS_BLOCK);
        if constexpr (UPPER)
            hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, X, ldx, y, offset, weight, upper, B, tail...);
        else
            hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, X, ldx, y, offset, weight, B, tail...);
    };
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {   // each launch with its chunk of the scalar
            const float *Ws = W + (int64_t)s0 * D, *lp = logtau + s0;
            launch_pass_shape(
                rows, D,
                [&] {
                    if constexpr (UPPER) go(scalar_upper_pass_mfma_kernel<LINK>, Ws, lp, sg, slab, g.n_iter);
                    else if constexpr (PARAM) go(scalar_par_pass_mfma_kernel<LINK>, Ws, lp, sg, slab, g.n_iter, par);
                    else go(scalar_pass_mfma_kernel<LINK>, Ws, lp, sg, slab, g.n_iter);
                },
                [&](auto full) {
                    constexpr bool FULL = decltype(full)::value;
                    if constexpr (UPPER) go(scalar_upper_pass_kernel<LINK, FULL>, (int)D, Ws, lp, sg, slab, g.n_iter);
                    else if constexpr (PARAM)
                        go(scalar_par_pass_kernel<LINK, FULL>, (int)D, Ws, lp, sg, slab, g.n_iter, par);
                    else go(scalar_pass_kernel<LINK, FULL>, (int)D, Ws, lp, sg, slab, g.n_iter);
                });
        },
        [&](int s0) {
            hipLaunchKernelGGL(scalar_slab_reduce_kernel<LINK>, rgrid, dim3(RED_BLOCK), 0, ctx->stream,
                               (const float*)slab, g.n_blocks, (int)D, (int)S, s0, ell, G, T);
        });
}

// ---- the mean-field finish: NbModel of csrc/bsc_meanfield.h, tau in the place of its log-dispersion -----------------

template <int LINK>
__global__ __launch_bounds__(MF_BLOCK) void scalar_mf_scalars_kernel(NbModel a) { meanfield_scalars_body(a); }

template <int LINK>
__global__ __launch_bounds__(MF_BLOCK) void scalar_mf_coord_kernel(NbModel a) { meanfield_coord_body(a); }

// The checks, the next step's noise, the arguments and the two launches.  The likelihood enters through
// stats = [ell | G | T] alone, so F only says whose kernels these are.
template <class F>
int scalar_family_update(bsc_ctx* ctx, const char* who, const double* stats, const double* lam_in, double* lam_out,
                         double* m1, double* m2, const double* eps, const float* W, const float* logtau, int32_t D,
                         int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                         double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                         double* eps_next, int32_t eps_next_ready, float* W_next, float* logtau_next, double* elbo,
                         double* grad) {
    constexpr int LINK = F::GLM_ID;
    BSC_REQUIRE(stats, "%s: stats is null (pending pass partials are not read: pass [ell | G | T])", who);
    int rc = check_meanfield_update(who, lam_in && lam_out && m1 && m2 && eps && W && logtau && elbo && grad, lam_in,
                                    lam_out, D, S, MF_MAX_S, prior_precision, /*has_gamma=*/true, a0, b0, scale, t);
    if (rc != BSC_OK) return rc;
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, logtau, eps_next, W_next, logtau_next, D, S, seed,
                         next_step, eps_next_ready);
    if (rc != BSC_OK) return rc;
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (NbModel::N_SLOTS * MF_MAX_S + 8) * sizeof(double), &ws);
    if (rc != BSC_OK) return rc;
    NbModel a;
    a.stats = stats; a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.logphi = logtau; a.eps_next = eps_next; a.W_next = W_next; a.logphi_next = logtau_next;
    a.scal = (double*)ws; a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S; a.P = D + 1;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) + a0 * log(b0) - lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    ctx->slab_rows = 0;   // the workspace is this finish's now
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish, timed apart from the pass
        hipLaunchKernelGGL(scalar_mf_scalars_kernel<LINK>, dim3(S + 1), dim3(MF_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(scalar_mf_coord_kernel<LINK>, dim3((a.P + MF_BLOCK - 1) / MF_BLOCK), dim3(MF_BLOCK), 0,
                           ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

// ---- the predictive -------------------------------------------------------------------------------------------------

// FULL: D == 256.  offset may be null.
template <int FAMILY, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void scalar_predict_kernel(PredictArgs a, const float* __restrict__ offset) {
    predict_body<PredictFamily<FAMILY>, NC, FULL, true>(a, offset);
}

// ... and upper is set
template <int FAMILY, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void scalar_upper_predict_kernel(PredictArgs a,
                                                                          const float* __restrict__ offset,
                                                                          const float* __restrict__ upper) {
    predict_body<PredictFamily<FAMILY>, NC, FULL, true, false, true>(a, offset, PredictGroups{}, upper);
}

// ... or the family's per-model constant `par` (F::PARAM)
template <int FAMILY, int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void scalar_par_predict_kernel(PredictArgs a, const float* __restrict__ offset,
                                                                        float par) {
    predict_body<PredictFamily<FAMILY>, NC, FULL, true>(a, offset, PredictGroups{}, nullptr, PredictOrdinal{}, par);
}

template <int FAMILY>
__global__ __launch_bounds__(BSC_WAVE) void scalar_predict_sum_kernel(const double* __restrict__ partial, int n,
                                                                      double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int FAMILY, bool UPPER, bool PARAM, int NC>
void launch_scalar_predict(bsc_ctx* ctx, const PredictArgs& a, const float* offset, const float* upper, float par,
                           int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    const auto go = [&](auto full) {
        constexpr bool FULL = decltype(full)::value;
        if constexpr (UPPER)
            hipLaunchKernelGGL((scalar_upper_predict_kernel<FAMILY, NC, FULL>), grid, block, 0, ctx->stream, a, offset,
                               upper);
        else if constexpr (PARAM)
            hipLaunchKernelGGL((scalar_par_predict_kernel<FAMILY, NC, FULL>), grid, block, 0, ctx->stream, a, offset,
                               par);
        else
            hipLaunchKernelGGL((scalar_predict_kernel<FAMILY, NC, FULL>), grid, block, 0, ctx->stream, a, offset);
    };
    if (a.D == WCOLS) go(std::true_type{});
    else go(std::false_type{});
}

// The predictive entry point `who` of a family with a per-draw scalar of its own (`logtau` [S], named `what` in the
// messages) and an offset that may be null.  UPPER: `upper` (not null) rides with the offset; without the flag it is
// not read.  PARAM: `par`, the family's per-model constant (checked by the entry point), is the kernels' last argument.
template <class F, bool UPPER = false, bool PARAM = false>
int scalar_family_predict_pass(bsc_ctx* ctx, const char* who, const char* what, const float* X, int64_t ldx,
                               const float* y, const float* upper, const float* offset, int64_t B, int32_t D,
                               const float* W, const float* logtau, int32_t S, float* mean, float* var, float* lpd,
                               double* lpd_sum, float par = 0.f) {
    constexpr int FAMILY = F::PREDICT_ID;
    static_assert(PARAM == F::PARAM && !(UPPER && PARAM), "the constant rides with the family that declares one");
    if constexpr (UPPER) BSC_REQUIRE((((uintptr_t)upper) & 3) == 0, "%s: upper must be 4-byte aligned", who);
    int rc = predict_check_batch(who, X, y, B, W, mean, var, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(logtau, "%s: %s is null", who, what);
    BSC_REQUIRE((((uintptr_t)offset) & 3) == 0 && (((uintptr_t)logtau) & 3) == 0,
                "%s: offset and %s must be 4-byte aligned", who, what);
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, y, B, D, W, logtau, S, mean, var, lpd, lpd_sum, &a, &n_blocks);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    {
        bsc_prof_scope prof(ctx);
        predict_launch_chunks(S, [&](auto nc) {
            launch_scalar_predict<FAMILY, UPPER, PARAM, decltype(nc)::value>(ctx, a, offset, upper, par, n_blocks);
        });
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(scalar_predict_sum_kernel<FAMILY>, dim3(1), dim3(BSC_WAVE), 0, ctx->stream,
                           (const double*)a.partial, n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // namespace
