// Interval and left censoring for the Weibull survival route (csrc/bsc_glm_weibull.hip): csrc/bsc_glm_pass.h's bodies with
// the per-draw scalar flag AND the upper-end flag on, their slab reduction, and csrc/bsc_predict_pass.h's body with the
// interval variant of its sixth family.  The finishes (bsc_glm_weibull_update, bsc_glm_scalar_fullrank_update) see
// [ell | G | T] alone and are shared as they are.  The kernels and the host side of the two entry points are
// csrc/bsc_scalar_family.h's `upper` variants (UPPER = true), with the Weibull family.
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
// one adds nothing -- by selects on the link's inputs (csrc/bsc_families.h).  Apart from that the link is NOT clamped:
// finite while z_a stays below about 88.
//
// A translation unit of its own so that every other one keeps its kernels, their names, their count and their code.
#include "bsc_scalar_family.h"

extern "C" {

int bsc_glm_weibull_data_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                       const float* offset, const float* weight, int64_t B, int32_t D, const float* W,
                                       const float* logshape, int32_t S, double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    if (!upper)   // the kernels of csrc/bsc_glm_weibull.hip: the same bits
        return bsc_glm_weibull_data_pass(ctx, X, ldx, y, offset, weight, B, D, W, logshape, S, ell, G, T);
    return scalar_family_data_pass<Weibull, true>(ctx, "bsc_glm_weibull_data_pass_interval", "logshape", X, ldx, y,
                                                  upper, offset, weight, B, D, W, logshape, S, ell, G, T);
}

int bsc_weibull_predict_pass_interval(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* upper,
                                      const float* offset, int64_t B, int32_t D, const float* W, const float* logshape,
                                      int32_t S, float* mean, float* var, float* lpd, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    if (!upper) return bsc_weibull_predict_pass(ctx, X, ldx, y, offset, B, D, W, logshape, S, mean, var, lpd, lpd_sum);
    return scalar_family_predict_pass<Weibull, true>(ctx, "bsc_weibull_predict_pass_interval", "logshape", X, ldx, y,
                                                     upper, offset, B, D, W, logshape, S, mean, var, lpd, lpd_sum);
}

}  // extern "C"
