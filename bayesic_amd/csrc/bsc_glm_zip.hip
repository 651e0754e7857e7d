// Zero-inflated Poisson regression with a learned inflation odds on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS
// bodies with the per-draw scalar flag on, their slab reduction, the finish for the latent z = [w (D) | tau]
// (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on e^tau has the negative binomial's form, so the finish is the
// same), and the predictive (csrc/bsc_predict_pass.h's body and envelope).  The kernels and the host side of the three
// entry points are csrc/bsc_scalar_family.h's, with the ZeroInflPoisson family (csrc/bsc_families.h).
//
//     y_n ~ ZIP(pi, mu_n):  with probability pi a structural zero, else Poisson(mu_n)
//     mu_n = e^{l_n},   l[n,s] = x_n . w_s + o_n   (the offset or log exposure as in the Poisson route)
//     w ~ N(0, I / prior_precision),   omega = pi / (1 - pi) = e^tau ~ Gamma(a0, b0)
// tau is the log ODDS of a structural zero, pi = sigmoid(tau), so that the prior on e^tau has the form the shared finish
// knows and T is the derivative with respect to the latent.  With u = tau + mu, L1 = log1p(omega) = softplus(tau):
//     y == 0:  log p = log(omega + e^{-mu}) - L1 = max(tau, -mu) + log1p(e^{-|u|}) - L1
//              d / d l = -mu sigmoid(-u),      d / d tau = sigmoid(u) (1 - pi) (1 - e^{-mu})
//     y > 0:   log p = y l - mu - L1           (-lnGamma(y + 1) left out in training, as in the Poisson route)
//              d / d l = y - mu,               d / d tau = -pi
// Per draw the pass leaves
//     ell[s] = sum_n v_n log p,     G[s,:] = sum_n r_ns x_n  (r = v d / d l),     T[s] = sum_n v_n d / d tau
// tau_s rides in the lanes as the dispersion of csrc/bsc_glm_nb.hip does (a lane owns one draw in both tile shapes); L1
// and pi are made once per launch in float64.  The block partials are NB_SLAB_STRIDE floats, reduced in float64 in a
// fixed order.  No float atomics anywhere: the same bits run to run.  NOT clamped, like the Poisson link: finite while
// e^l is.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_zip_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                          const float* weight, int64_t B, int32_t D, const float* W, const float* logodds, int32_t S,
                          double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<ZeroInflPoisson>(ctx, "bsc_glm_zip_data_pass", "logodds", X, ldx, y, nullptr, offset,
                                                    weight, B, D, W, logodds, S, ell, G, T);
}

int bsc_glm_zip_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                       double* m2, const double* eps, const float* W, const float* logodds, int32_t D, int32_t S,
                       double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                       double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                       int32_t eps_next_ready, float* W_next, float* logodds_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<ZeroInflPoisson>(ctx, "bsc_glm_zip_update", stats, lam_in, lam_out, m1, m2, eps, W,
                                                 logodds, D, S, scale, prior_precision, a0, b0, t, lr, beta1, beta2,
                                                 adam_eps, seed, next_step, eps_next, eps_next_ready, W_next,
                                                 logodds_next, elbo, grad);
}

int bsc_zip_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                         int32_t D, const float* W, const float* logodds, int32_t S, float* mean, float* var,
                         float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<ZeroInflPoisson>(ctx, "bsc_zip_predict_pass", "logodds", X, ldx, y, nullptr,
                                                       offset, B, D, W, logodds, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
