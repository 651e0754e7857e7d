// Log-normal survival regression (accelerated failure time) with right censoring and a learned scale on the fused
// pathwise pass: csrc/bsc_glm_pass.h's OBS bodies with the per-draw scalar flag on, their slab reduction, the finish for
// the latent z = [w (D) | tau] (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on e^tau has the negative
// binomial's form, so the finish is the same), and the predictive (csrc/bsc_predict_pass.h's body and envelope).  The
// kernels and the host side of the three entry points are csrc/bsc_scalar_family.h's, with the LogNormal family
// (csrc/bsc_families.h).
//
//     t_n ~ LogNormal(location l_n, scale sigma),   l[n,s] = x_n . w_s + o_n
//     w ~ N(0, I / prior_precision),   k = 1 / sigma = e^tau ~ Gamma(a0, b0)
//     delta_n = 1: the event was seen at t_n;   delta_n = 0: right-censored, the event is later than t_n
// tau is the log of the INVERSE scale, so that the prior on e^tau has the form the shared finish knows and T is the
// derivative with respect to the latent.  The censoring flag rides in the sign of y, as in csrc/bsc_glm_weibull.hip:
// y_n > 0 is an event at y_n, y_n < 0 is censored at -y_n; 0, NaN and infinity are invalid and are the caller's to keep
// out (a row of weight 0 may hold them).  With t = |y|, delta = (y > 0), ly = log t, z = k (ly - l) and
// h(z) = phi(z) / Phi(-z), the hazard of the standard normal:
//     log f(t) = tau - ly - z^2 / 2 - log(2 pi) / 2,     log S(t) = log Phi(-z)
// Per draw the pass leaves
//     ell[s] = sum_n v_n [ delta_n log f + (1 - delta_n) log Phi(-z_ns) ]               (the full density)
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n k_s [ delta_n z_ns + (1 - delta_n) h(z_ns) ]
//     T[s]   = sum_n v_n [ delta_n (1 - z_ns^2) - (1 - delta_n) z_ns h(z_ns) ]          (= d ell[s] / d tau_s)
// l is the location of log t, not the log mean: E t = e^{l + sigma^2 / 2}.  tau_s rides in the lanes as the dispersion
// of csrc/bsc_glm_nb.hip does (a lane owns one draw in both tile shapes); the density has no per-draw constant.  A
// censored row needs log Phi(-z) and h(z) per (row, draw), accurate in both tails: csrc/bsc_special_f32.h's
// bsc_lognormsf_hazard_f32, one scaled complementary error function for both.  The block partials are NB_SLAB_STRIDE
// floats, reduced in float64 in a fixed order.  No float atomics anywhere: the same bits run to run.  NOT clamped, and
// nothing to clamp: every term is finite for every finite z whose square is.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_lognormal_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                                const float* weight, int64_t B, int32_t D, const float* W, const float* loginvscale,
                                int32_t S, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<LogNormal>(ctx, "bsc_glm_lognormal_data_pass", "loginvscale", X, ldx, y, nullptr,
                                              offset, weight, B, D, W, loginvscale, S, ell, G, T);
}

int bsc_glm_lognormal_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                             double* m2, const double* eps, const float* W, const float* loginvscale, int32_t D,
                             int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                             double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                             double* eps_next, int32_t eps_next_ready, float* W_next, float* loginvscale_next,
                             double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<LogNormal>(ctx, "bsc_glm_lognormal_update", stats, lam_in, lam_out, m1, m2, eps, W,
                                           loginvscale, D, S, scale, prior_precision, a0, b0, t, lr, beta1, beta2,
                                           adam_eps, seed, next_step, eps_next, eps_next_ready, W_next,
                                           loginvscale_next, elbo, grad);
}

int bsc_lognormal_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                               int64_t B, int32_t D, const float* W, const float* loginvscale, int32_t S, float* mean,
                               float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<LogNormal>(ctx, "bsc_lognormal_predict_pass", "loginvscale", X, ldx, y, nullptr,
                                                 offset, B, D, W, loginvscale, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
