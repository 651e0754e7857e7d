// Beta regression (logit link) with a learned precision on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies
// with the per-draw scalar flag on and the sixth link, their slab reduction, the finish for the latent z = [w (D) | tau]
// (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on the scalar has the negative binomial's form, so the finish
// is the same), and the predictive (csrc/bsc_predict_pass.h's body and envelope with its eighth family).  The kernels and
// the host side of the three entry points are csrc/bsc_scalar_family.h's, with the Beta family.
//
//     y_n ~ Beta(a_n, b_n),  0 < y_n < 1,  a_n = m_n phi,  b_n = (1 - m_n) phi
//     m_n = sigmoid(l_n),  E y_n = m_n,  Var y_n = m_n (1 - m_n) / (1 + phi)
//     l[n,s] = x_n . w_s + o_n,   w ~ N(0, I / prior_precision),   phi = e^tau ~ Gamma(a0, b0)
// With ly = log y and l1y = log1p(-y):
//     log p(y | l, phi) = lnGamma(phi) - lnGamma(a) - lnGamma(b) + (a - 1) ly + (b - 1) l1y      (nothing left out)
// Per draw the pass leaves
//     ell[s] = sum_n v_n log p(y_n | l_ns, phi_s)
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n phi_s m (1 - m) [ (ly - l1y) - psi(a) + psi(b) ]
//     T[s]   = sum_n v_n phi_s [ psi(phi_s) + m (ly - psi(a)) + (1 - m)(l1y - psi(b)) ]      (= d ell[s] / d tau_s)
// tau_s rides in the lanes as the dispersion of csrc/bsc_glm_nb.hip does (a lane owns one draw in both tile shapes);
// lnGamma(phi_s) and psi(phi_s) are made once per launch in float64 and rounded.  lnGamma and psi at a and at b change
// with every (row, draw) and run towards 0 as the logit grows: csrc/bsc_special_f32.h's bsc_lgamma_psi_f32, a shifted
// product of at most eight factors and three asymptotic terms, evaluated twice, one after the other.  m and 1 - m come
// EACH from the stable logistic form (e / (1 + e) and 1 / (1 + e), e = exp(-|l|)), never 1 - m by subtraction.  The block
// partials are NB_SLAB_STRIDE floats, reduced in float64 in a fixed order.  No float atomics anywhere: the same bits run
// to run.  NOT clamped: finite while m phi and its reciprocal are normal float32 values (|l| <= 80 at tau in [-2, 5]).
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_beta_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                           const float* weight, int64_t B, int32_t D, const float* W, const float* logprec, int32_t S,
                           double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_data_pass<Beta>(ctx, "bsc_glm_beta_data_pass", "logprec", X, ldx, y, nullptr, offset, weight,
                                         B, D, W, logprec, S, ell, G, T);
}

int bsc_glm_beta_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                        double* m2, const double* eps, const float* W, const float* logprec, int32_t D, int32_t S,
                        double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                        double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                        int32_t eps_next_ready, float* W_next, float* logprec_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<Beta>(ctx, "bsc_glm_beta_update", stats, lam_in, lam_out, m1, m2, eps, W, logprec, D, S,
                                      scale, prior_precision, a0, b0, t, lr, beta1, beta2, adam_eps, seed, next_step,
                                      eps_next, eps_next_ready, W_next, logprec_next, elbo, grad);
}

int bsc_beta_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                          int32_t D, const float* W, const float* logprec, int32_t S, float* mean, float* var,
                          float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_predict_pass<Beta>(ctx, "bsc_beta_predict_pass", "logprec", X, ldx, y, nullptr, offset, B, D,
                                            W, logprec, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
