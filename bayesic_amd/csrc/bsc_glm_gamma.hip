// Gamma regression (log link) with a learned shape on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies with the
// per-draw scalar flag on and the fourth link, their slab reduction, the finish for the latent z = [w (D) | tau]
// (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on the scalar has the negative binomial's form, so the finish
// is the same), and the predictive (csrc/bsc_predict_pass.h's body and envelope with its fifth family).  The kernels and
// the host side of the three entry points are csrc/bsc_scalar_family.h's, with the Gamma family.
//
//     y_n ~ Gamma(shape alpha, rate alpha / mu_n),  y_n > 0,  E y_n = mu_n = exp(l_n),  Var y_n = mu_n^2 / alpha
//     l[n,s] = x_n . w_s + o_n,   w ~ N(0, I / prior_precision),   alpha = e^tau ~ Gamma(a0, b0)
// With ly = log y, c_a(alpha) = alpha log alpha - lnGamma(alpha) and c_1(alpha) = log alpha + 1 - psi(alpha):
//     log p(y | l, alpha) = c_a + alpha (ly - l - y e^{-l}) - ly                (the full density, nothing left out)
// Per draw the pass leaves
//     ell[s] = sum_n v_n log p(y_n | l_ns, alpha_s)
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n alpha_s (y_n e^{-l_ns} - 1)
//     T[s]   = sum_n v_n alpha_s (c_1 + ly_n - l_ns - y_n e^{-l_ns})                         (= d ell[s] / d tau_s)
// tau_s rides in the lanes as the dispersion of csrc/bsc_glm_nb.hip does (a lane owns one draw in both tile shapes);
// c_a and c_1 are made once per launch in float64 and rounded, so the link is one exp, one log and a few FMAs per
// (row, draw).  The block partials are NB_SLAB_STRIDE floats, reduced in float64 in a fixed order.  No float atomics
// anywhere: the same bits run to run.  NOT clamped: finite while y e^{-l} is below the float32 maximum.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_gamma_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                            const float* weight, int64_t B, int32_t D, const float* W, const float* logshape,
                            int32_t S, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<Gamma>(ctx, "bsc_glm_gamma_data_pass", "logshape", X, ldx, y, nullptr, offset,
                                          weight, B, D, W, logshape, S, ell, G, T);
}

int bsc_glm_gamma_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                         double* m2, const double* eps, const float* W, const float* logshape, int32_t D, int32_t S,
                         double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                         double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                         int32_t eps_next_ready, float* W_next, float* logshape_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<Gamma>(ctx, "bsc_glm_gamma_update", stats, lam_in, lam_out, m1, m2, eps, W, logshape, D,
                                       S, scale, prior_precision, a0, b0, t, lr, beta1, beta2, adam_eps, seed,
                                       next_step, eps_next, eps_next_ready, W_next, logshape_next, elbo, grad);
}

int bsc_gamma_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                           int32_t D, const float* W, const float* logshape, int32_t S, float* mean, float* var,
                           float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<Gamma>(ctx, "bsc_gamma_predict_pass", "logshape", X, ldx, y, nullptr, offset, B,
                                             D, W, logshape, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
