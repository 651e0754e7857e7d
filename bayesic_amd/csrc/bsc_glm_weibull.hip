// Weibull survival regression (accelerated failure time) with right censoring and a learned shape on the fused pathwise
// pass: csrc/bsc_glm_pass.h's OBS bodies with the per-draw scalar flag on and the fifth link, their slab reduction, the
// finish for the latent z = [w (D) | tau] (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on the scalar has the
// negative binomial's form, so the finish is the same), and the predictive (csrc/bsc_predict_pass.h's body and envelope
// with its sixth family).  The kernels and the host side of the three entry points are csrc/bsc_scalar_family.h's, with
// the Weibull family (csrc/bsc_families.h).
//
//     t_n ~ Weibull(shape k, scale e^{l_n}),   l[n,s] = x_n . w_s + o_n
//     w ~ N(0, I / prior_precision),   k = e^tau ~ Gamma(a0, b0)
//     delta_n = 1: the event was seen at t_n;   delta_n = 0: right-censored, the event is later than t_n
// The censoring flag rides in the sign of y, free because a duration is positive: y_n > 0 is an event at y_n, y_n < 0 is
// censored at -y_n; 0, NaN and infinity are invalid and are the caller's to keep out (a row of weight 0 may hold them).
// With t = |y|, delta = (y > 0), ly = log t and z = k (ly - l):
//     log f(t) = tau + z - ly - e^z,     log S(t) = -e^z
// Per draw the pass leaves
//     ell[s] = sum_n v_n [ delta_n (tau_s + z_ns - ly_n) - e^{z_ns} ]
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n k_s (e^{z_ns} - delta_n)
//     T[s]   = sum_n v_n [ delta_n (1 + z_ns) - z_ns e^{z_ns} ]                               (= d ell[s] / d tau_s)
// l is the log SCALE, not the log mean: E t = e^l Gamma(1 + 1/k).  tau_s rides in the lanes as the dispersion of
// csrc/bsc_glm_nb.hip does (a lane owns one draw in both tile shapes); the density has no per-draw constant, so the link
// is one log, one exp and a few FMAs per (row, draw), and the flag is a select.  The block partials are NB_SLAB_STRIDE
// floats, reduced in float64 in a fixed order.  No float atomics anywhere: the same bits run to run.  NOT clamped, like
// the Poisson and Gamma links: finite while z stays below about 88.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_weibull_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                              const float* weight, int64_t B, int32_t D, const float* W, const float* logshape,
                              int32_t S, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<Weibull>(ctx, "bsc_glm_weibull_data_pass", "logshape", X, ldx, y, nullptr, offset,
                                            weight, B, D, W, logshape, S, ell, G, T);
}

int bsc_glm_weibull_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                           double* m2, const double* eps, const float* W, const float* logshape, int32_t D, int32_t S,
                           double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                           double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                           double* eps_next, int32_t eps_next_ready, float* W_next, float* logshape_next, double* elbo,
                           double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<Weibull>(ctx, "bsc_glm_weibull_update", stats, lam_in, lam_out, m1, m2, eps, W,
                                         logshape, D, S, scale, prior_precision, a0, b0, t, lr, beta1, beta2, adam_eps,
                                         seed, next_step, eps_next, eps_next_ready, W_next, logshape_next, elbo, grad);
}

int bsc_weibull_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                             int32_t D, const float* W, const float* logshape, int32_t S, float* mean, float* var,
                             float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<Weibull>(ctx, "bsc_weibull_predict_pass", "logshape", X, ldx, y, nullptr, offset,
                                               B, D, W, logshape, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
