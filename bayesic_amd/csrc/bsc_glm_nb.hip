// Negative-binomial regression with a learned dispersion on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies
// with the dispersion flag on, their slab reduction, the finish for the latent z = [w (D) | tau] (csrc/bsc_meanfield.h's
// bodies with NbModel), and the predictive (csrc/bsc_predict_pass.h's body and envelope with its fourth family).  The
// kernels and the host side of the three entry points are csrc/bsc_scalar_family.h's, with the NegBin family.
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
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_nb_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                         const float* weight, int64_t B, int32_t D, const float* W, const float* logphi, int32_t S,
                         double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<NegBin>(ctx, "bsc_glm_nb_data_pass", "logphi", X, ldx, y, nullptr, offset, weight, B,
                                           D, W, logphi, S, ell, G, T);
}

int bsc_glm_nb_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                      const double* eps, const float* W, const float* logphi, int32_t D, int32_t S, double scale,
                      double prior_precision, double a0, double b0, int64_t t, double lr, double beta1, double beta2,
                      double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                      float* W_next, float* logphi_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<NegBin>(ctx, "bsc_glm_nb_update", stats, lam_in, lam_out, m1, m2, eps, W, logphi, D, S,
                                        scale, prior_precision, a0, b0, t, lr, beta1, beta2, adam_eps, seed, next_step,
                                        eps_next, eps_next_ready, W_next, logphi_next, elbo, grad);
}

int bsc_nb_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                        int32_t D, const float* W, const float* logphi, int32_t S, float* mean, float* var, float* lpd,
                        double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<NegBin>(ctx, "bsc_nb_predict_pass", "logphi", X, ldx, y, nullptr, offset, B, D, W,
                                              logphi, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
