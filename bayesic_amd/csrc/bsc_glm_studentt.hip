// Student-t robust regression with a learned scale and fixed degrees of freedom on the fused pathwise pass:
// csrc/bsc_glm_pass.h's OBS bodies with the per-draw scalar flag on, their slab reduction, the finish for the latent
// z = [w (D) | tau] (csrc/bsc_meanfield.h's bodies with NbModel -- the prior on e^tau has the negative binomial's form, so
// the finish is the same), and the predictive (csrc/bsc_predict_pass.h's body and envelope).  The kernels and the host
// side of the three entry points are csrc/bsc_scalar_family.h's, with the StudentT family (csrc/bsc_families.h).
//
//     y_n ~ StudentT(df = nu, location l_n, scale sigma),   l[n,s] = x_n . w_s + o_n
//     w ~ N(0, I / prior_precision),   k = 1 / sigma = e^tau ~ Gamma(a0, b0),   nu > 0 fixed by the caller
// tau is the log of the INVERSE scale, as in csrc/bsc_glm_lognormal.hip, so that the prior on e^tau has the form the shared
// finish knows and T is the derivative with respect to the latent.  y is any finite float.  With z = k (y - l) and
// c_nu = lnGamma((nu + 1) / 2) - lnGamma(nu / 2) - log(nu pi) / 2:
//     log p = tau + c_nu - ((nu + 1) / 2) log1p(z^2 / nu)
// Per draw the pass leaves
//     ell[s] = sum_n v_n log p(y_n | l_ns, k_s)                                          (the full density)
//     G[s,:] = sum_n r_ns x_n,     r_ns = v_n k_s (nu + 1) z_ns / (nu + z_ns^2)
//     T[s]   = sum_n v_n nu (1 - z_ns^2) / (nu + z_ns^2)                                 (= d ell[s] / d tau_s)
// The residual is bounded in z -- at most k (nu + 1) / (2 sqrt nu), at z^2 = nu, and falling like 1 / z beyond -- which is
// what keeps one gross outlier from moving the fit; the Gaussian's residual k z is not.
// nu is the first per-MODEL constant a family carries down to its link.  It is no field of a struct the other units
// share and no argument of their kernels: this unit's pass and predictive kernels are the scalar_par_* templates of
// csrc/bsc_scalar_family.h, which take it as one float behind their other arguments and hand it to the family's
// glm_disp / predict_slots.  There c_nu is made once per launch in float64 (bsc_lgamma_f64) and tau_s, k_s, tau_s + c_nu
// and nu ride in the lane's four registers as the dispersion of csrc/bsc_glm_nb.hip does.  nu is rounded to float32 where
// it enters (1, 2.5, 4, 30 and 1e6 are exact) and c_nu is made from the rounded value, so the density is normalised for
// the nu the link uses.  The block partials are NB_SLAB_STRIDE floats, reduced in float64 in a fixed order.  No float
// atomics anywhere: the same bits run to run.  NOT clamped, and nothing to clamp: every term is finite while z^2 is.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include <cmath>

#include "bsc_scalar_family.h"

namespace {

// The degrees of freedom of an entry point `who`: finite and > 0, and a normal float32, which is what the kernels take.
inline int check_df(const char* who, double df) {
    BSC_REQUIRE(std::isfinite(df) && df > 0.0, "%s: df=%g must be finite and > 0", who, df);
    BSC_REQUIRE(df >= 1.17549435e-38 && df <= 3.40282347e38, "%s: df=%g is outside the float32 range", who, df);
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_glm_studentt_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                               const float* weight, int64_t B, int32_t D, const float* W, const float* loginvscale,
                               int32_t S, double df, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    const int rc = check_df("bsc_glm_studentt_data_pass", df);
    if (rc != BSC_OK) return rc;
    return scalar_family_data_pass<StudentT, false, true>(ctx, "bsc_glm_studentt_data_pass", "loginvscale", X, ldx, y,
                                                          nullptr, offset, weight, B, D, W, loginvscale, S, ell, G, T,
                                                          (float)df);
}

int bsc_glm_studentt_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, const float* loginvscale, int32_t D,
                            int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t, double lr,
                            double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                            double* eps_next, int32_t eps_next_ready, float* W_next, float* loginvscale_next,
                            double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return scalar_family_update<StudentT>(ctx, "bsc_glm_studentt_update", stats, lam_in, lam_out, m1, m2, eps, W,
                                          loginvscale, D, S, scale, prior_precision, a0, b0, t, lr, beta1, beta2,
                                          adam_eps, seed, next_step, eps_next, eps_next_ready, W_next,
                                          loginvscale_next, elbo, grad);
}

int bsc_studentt_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                              int64_t B, int32_t D, const float* W, const float* loginvscale, int32_t S, double df,
                              float* mean, float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const int rc = check_df("bsc_studentt_predict_pass", df);
    if (rc != BSC_OK) return rc;
    return scalar_family_predict_pass<StudentT, false, true>(ctx, "bsc_studentt_predict_pass", "loginvscale", X, ldx, y,
                                                             nullptr, offset, B, D, W, loginvscale, S, mean, var, lpd,
                                                             lpd_sum, (float)df);
}

}  // extern "C"
