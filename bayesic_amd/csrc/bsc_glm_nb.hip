// Negative-binomial regression with a learned dispersion on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies
// with the dispersion flag on, their slab reduction, the finish for the latent z = [w (D) | tau] (csrc/bsc_meanfield.h's
// bodies with NbModel below), and the predictive (csrc/bsc_predict_pass.h's body and envelope with its fourth family).
//
//     y_n ~ NegBin(mean exp(l_n), dispersion phi),  Var y_n = mu_n + mu_n^2 / phi,   l[n,s] = x_n . w_s + o_n
//     w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0)
// With u = l - tau_s the log-density is the logistic link at a shifted logit,
//     log p(y | l, phi) = lnGamma(y + phi) - lnGamma(phi) - lnGamma(y + 1) + y u - (y + phi) softplus(u)
// finite for every finite l (the Poisson link is not).  Per draw the pass leaves
//     ell[s] = sum_n v_n [ dlnGamma(y_n, phi_s) + y_n u - (y_n + phi_s) softplus(u) ]
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n [ y_n - (y_n + phi_s) sigmoid(u) ]
//     T[s]   = sum_n v_n [ phi_s dpsi(y_n, phi_s) - phi_s softplus(u) ] - sum_n r_ns          (= d ell[s] / d tau_s)
// tau_s rides in the lanes (a lane owns one draw in both tile shapes), lnGamma and psi of y + phi are float32 per
// (row, draw) (csrc/bsc_special_f32.h), and T is one more lane accumulator: the block partials are NB_SLAB_STRIDE =
// REG_SLAB_G + 16 floats, ell at [SLAB_G + s], T at [SLAB_G + 8 + s], reduced in float64 in a fixed order as the other
// passes' are.  No float atomics anywhere: the same bits run to run.
//
// A translation unit of its own so that the kernels of csrc/bsc_glm.hip, bsc_glm_obs.hip, bsc_glm_group.hip,
// bsc_predict.hip and bsc_predict_offset.hip keep their names, their count and their code.
#include "bsc_glm_pass.h"
#include "bsc_meanfield.h"
#include "bsc_predict_pass.h"

namespace {

constexpr int MAX_S = 64;

// ---- the pass ---------------------------------------------------------------------------------------------------------

template <bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_nb_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, const float* __restrict__ logphi, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_body<GLM_NEGBIN, FULL, true, false, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr, logphi);
}

__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_nb_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, const float* __restrict__ logphi, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GLM_NEGBIN, true, false, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logphi);
}

__global__ __launch_bounds__(RED_BLOCK) void glm_nb_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                       int D, int S, int s_base,
                                                                       double* __restrict__ ell, double* __restrict__ G,
                                                                       double* __restrict__ T) {
    regress_slab_reduce<NB_SLAB_STRIDE>(slab, n_blocks, D, S, s_base, ell, G, T);
}

// ---- the finish -------------------------------------------------------------------------------------------------------

// z = [w (D) | tau]; scal = [g_tau (64) | f (64) | sum rho]; c0 = D/2 log(prec / 2 pi) + a0 log b0 - lnGamma(a0).
struct NbModel : MeanfieldArgs {
    const float* logphi;     // [S]
    float* logphi_next;

    static constexpr int N_SLOTS = 2;
    static constexpr bool LAST_HAS_NEXT = true;

    static __device__ __forceinline__ double extra_sq(const NbModel&, int, double*) { return 0.0; }

    // g_tau and f_s = scale ell_s + log p(z_s) with tau_s the float32 value the pass read; T sits behind G in stats
    static __device__ __forceinline__ void draw_scalars(const NbModel& a, int s, double wsq, double) {
        const int D = a.D, S = a.S;
        const double tau = (double)a.logphi[s];
        const double phi = exp(tau);
        const double T = a.stats[S + (int64_t)S * D + s];
        a.scal[s] = a.scale * T + a.a0 - a.b0 * phi;
        a.scal[MF_MAX_S + s] = a.scale * a.stats[s] + a.c0 - 0.5 * a.prec * wsq + a.a0 * tau - a.b0 * phi;
    }

    static __device__ __forceinline__ double grad_term(const NbModel& a, int, int s) { return a.scal[s]; }

    static __device__ __forceinline__ void store_next(const NbModel& a, int i, double nm, double sd) {
        const int S = a.S, P = a.P;
        for (int s = 0; s < S; ++s) a.logphi_next[s] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
    }
};

__global__ __launch_bounds__(MF_BLOCK) void glm_nb_scalars_kernel(NbModel a) { meanfield_scalars_body(a); }

__global__ __launch_bounds__(MF_BLOCK) void glm_nb_coord_kernel(NbModel a) { meanfield_coord_body(a); }

// ---- the predictive ---------------------------------------------------------------------------------------------------

// FULL: D == 256.  offset may be null.
template <int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_nb_kernel(PredictArgs a, const float* __restrict__ offset) {
    predict_body<PREDICT_NEGBIN, NC, FULL, true>(a, offset);
}

__global__ __launch_bounds__(BSC_WAVE) void predict_nb_sum_kernel(const double* __restrict__ partial, int n,
                                                                  double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int NC>
void launch_predict_nb_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS) hipLaunchKernelGGL((predict_nb_kernel<NC, true>), grid, block, 0, ctx->stream, a, offset);
    else hipLaunchKernelGGL((predict_nb_kernel<NC, false>), grid, block, 0, ctx->stream, a, offset);
}

}  // namespace

extern "C" {

int bsc_glm_nb_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                         const float* weight, int64_t B, int32_t D, const float* W, const float* logphi, int32_t S,
                         double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_nb_data_pass";
    const int rc0 = check_glm_obs_args(who, BSC_GLM_LOGISTIC, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc0 != BSC_OK) return rc0;
    BSC_REQUIRE(logphi, "%s: logphi is null", who);
    BSC_REQUIRE((((uintptr_t)logphi) & 3) == 0, "%s: logphi must be 4-byte aligned", who);
    BSC_REQUIRE(ell && G && T, "%s: null output", who);

    const int rows = pass_rows(D, y, offset, weight);
    const PassGrid g = pass_grid(ctx, B, rows);
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * NB_SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    const dim3 rgrid((NB_SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, offset, weight, B,
                           tail...);
    };
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {   // each launch with its chunk of logphi
            const float *Ws = W + (int64_t)s0 * D, *lp = logphi + s0;
            launch_pass_shape(
                rows, D, [&] { go(glm_nb_pass_mfma_kernel, Ws, lp, sg, slab, g.n_iter); },
                [&](auto full) { go(glm_nb_pass_kernel<decltype(full)::value>, (int)D, Ws, lp, sg, slab, g.n_iter); });
        },
        [&](int s0) {
            hipLaunchKernelGGL(glm_nb_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, (const float*)slab,
                               g.n_blocks, (int)D, (int)S, s0, ell, G, T);
        });
}

int bsc_glm_nb_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                      const double* eps, const float* W, const float* logphi, int32_t D, int32_t S, double scale,
                      double prior_precision, double a0, double b0, int64_t t, double lr, double beta1, double beta2,
                      double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                      float* W_next, float* logphi_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_nb_update";
    BSC_REQUIRE(stats, "%s: stats is null (pending pass partials are not read: pass [ell | G | T])", who);
    int rc = check_meanfield_update(who, lam_in && lam_out && m1 && m2 && eps && W && logphi && elbo && grad, lam_in,
                                    lam_out, D, S, MAX_S, prior_precision, /*has_gamma=*/true, a0, b0, scale, t);
    if (rc != BSC_OK) return rc;
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, logphi, eps_next, W_next, logphi_next, D, S, seed,
                         next_step, eps_next_ready);
    if (rc != BSC_OK) return rc;
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (NbModel::N_SLOTS * MAX_S + 8) * sizeof(double), &ws);
    if (rc != BSC_OK) return rc;
    NbModel a;
    a.stats = stats; a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.logphi = logphi; a.eps_next = eps_next; a.W_next = W_next; a.logphi_next = logphi_next;
    a.scal = (double*)ws; a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S; a.P = D + 1;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) + a0 * log(b0) - lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    ctx->slab_rows = 0;   // the workspace is this finish's now
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish, timed apart from the pass
        hipLaunchKernelGGL(glm_nb_scalars_kernel, dim3(S + 1), dim3(MF_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(glm_nb_coord_kernel, dim3((a.P + MF_BLOCK - 1) / MF_BLOCK), dim3(MF_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_nb_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                        int32_t D, const float* W, const float* logphi, int32_t S, float* mean, float* var, float* lpd,
                        double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_nb_predict_pass";
    int rc = predict_check_batch(who, X, y, B, W, mean, var, lpd, lpd_sum);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(logphi, "%s: logphi is null", who);
    BSC_REQUIRE((((uintptr_t)offset) & 3) == 0 && (((uintptr_t)logphi) & 3) == 0,
                "%s: offset and logphi must be 4-byte aligned", who);
    PredictArgs a;
    int n_blocks = 0;
    rc = predict_setup(ctx, who, X, ldx, y, B, D, W, logphi, S, mean, var, lpd, lpd_sum, &a, &n_blocks);
    if (rc != BSC_OK || n_blocks == 0) return rc;
    {
        bsc_prof_scope prof(ctx);
        predict_launch_chunks(S, [&](auto nc) { launch_predict_nb_nc<decltype(nc)::value>(ctx, a, offset, n_blocks); });
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(predict_nb_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream, (const double*)a.partial,
                           n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
