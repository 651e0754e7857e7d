// Full-covariance Gaussian guide for the regression families with ONE learned scalar behind the weights (negative
// binomial: dispersion, Gamma and Weibull: shape; csrc/bsc_glm_nb.hip, bsc_glm_gamma.hip, bsc_glm_weibull.hip): the
// finish of one update.
//
// q(z) = N(mu, L L^T) over z = [w (D) | tau], P = D + 1, L lower-triangular with L_ii = e^{rho_i}.
// lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal (P(P+1)/2)]; row i starts at P + i(i+1)/2 and
// its diagonal slot holds rho_i: csrc/bsc_blr_full.hip's layout.  The three data passes (unchanged) give ell_s, G_s and
// T_s = d ell_s / d tau_s for the draws (W_s, tau_s); the likelihood enters through them alone, so ONE kernel serves
// the three families.  Under w ~ N(0, I / prec), e^tau ~ Gamma(a0, b0) (NbModel of csrc/bsc_meanfield.h):
//     g_si        = scale G_si - prec W_si   (i < D)     (W_s: the float32-rounded draw the pass read)
//     g_sD        = scale T_s + a0 - b0 e^{tau_s}        (tau_s: the float32 value the pass read)
//     f_s         = scale ell_s + c0 - prec/2 |w_s|^2 + a0 tau_s - b0 e^{tau_s}
//     d / d mu    = mean_s g_s
//     d / d L_ij  = mean_s g_si eps_sj                   (j < i)
//     d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
//     ELBO        = mean_s f_s + sum_i rho_i + P/2 (1 + log 2 pi)
//     c0          = D/2 log(prec / 2 pi) + a0 log b0 - lnGamma(a0)
// then Adam ascent on every entry (bsc_adam_ascent) and the next draw z'_s = mu' + L' eps'_s.
//
// Rows of L are independent (g_si needs column i of G and W, or T and tau for the last row), so workgroup k owns rows k
// and P-1-k (k + 1 and P - k entries: P + 1 together); P is odd, so the middle row D/2 is a workgroup of its own:
// (P + 1) / 2 workgroups of equal work.  Workgroup 0 owns the tau row, |w_s|^2, sum rho and the ELBO.  Each workgroup
// forms its rows of the next draw from its own rows of L'.  Every sum runs in a fixed order, no atomics, no
// inter-workgroup communication: the result is the same bytes run to run.  The caller double-buffers lam and the
// draws.  Small and latency-bound: every load of the prologue is issued unconditionally from a clamped index, so that
// none of them sits in a branch of its own behind a wait (the rule of the regression finish, csrc/bsc_blr.hip).
#include "bsc_fullrank.h"

// as the other full-rank finishes: no contraction into FMAs.  With a diagonal L this is the mean-field finish's
// arithmetic (csrc/bsc_meanfield.h) but for the order of the |w_s|^2 and sum rho sums: the two agree to rtol 1e-12.
#pragma clang fp contract(off)

namespace {

constexpr int SF_MAX_D = 256;
constexpr int SF_MAX_P = SF_MAX_D + 1;

struct GlmScalarFullArgs {
    const double* stats;       // [ell (S) | G (S*D) | T (S)]
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;         // [S, P] (bsc_blr_noise's layout, every column read)
    const float* W;            // [S, D]
    const float* logscalar;    // [S]
    const double* eps_next;    // nullptr: no next draw
    float* W_next;
    float* logscalar_next;
    double* elbo;
    double* grad;              // lam's layout
    int D, S;
    double scale, prec, a0, b0;
    double c0;                 // D/2 log(prec / 2 pi) + a0 log b0 - lnGamma(a0)
    bsc_adam adam;
};

__global__ __launch_bounds__(FR_BLOCK) void glm_scalar_fullrank_update_kernel(GlmScalarFullArgs a) {
    __shared__ double wsq[FR_MAX_S];       // |w_s|^2, then f_s (workgroup 0)
    __shared__ double gs[2][FR_MAX_S];     // g_{s,i} of the two rows
    __shared__ double Lnew[2][SF_MAX_P];   // the rows of L' (diagonal as e^{rho'})
    __shared__ double mu_new[2];
    __shared__ double rho_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S, P = D + 1;
    const fr_rows rp = fr_row_pair(blockIdx.x, P);
    const bool tau_wg = blockIdx.x == 0;   // owns row P-1 (tau) and the ELBO
    const double inv_S = 1.0 / (double)S;

    // ---- g_{s,i} for the rows of this workgroup: one (row, draw) per thread, every load from a clamped index ----
    const int n_g = rp.n_rows * S;                       // <= 128
    const int idx = tid < n_g ? tid : n_g - 1;
    const int gr = idx / S, gsmp = idx - gr * S, gi = gr ? rp.row1 : rp.row0;
    const int gic = gi < D ? gi : D - 1;
    const double Gv = a.stats[S + (int64_t)gsmp * D + gic];
    const double Wv = (double)a.W[(int64_t)gsmp * D + gic];
    const double Tv = a.stats[S + (int64_t)S * D + gsmp];
    const double ellv = a.stats[gsmp];
    const double tauv = (double)a.logscalar[gsmp];
    // sum rho: the last wave of workgroup 0 (a wave-uniform condition), P <= 257 diagonal slots in five strides
    double rv[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (tau_wg && wave == FR_WAVES - 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int i = lane + k * BSC_WAVE, ic = i < P ? i : P - 1;
            rv[k] = a.lam_in[P + ic * (ic + 1) / 2 + ic];
        }
    }
    if (tau_wg) {
        for (int s = wave; s < S; s += FR_WAVES) {
            double wv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = lane + k * BSC_WAVE, dc = d < D ? d : D - 1;
                wv[k] = (double)a.W[(int64_t)s * D + dc];
            }
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) part += lane + k * BSC_WAVE < D ? wv[k] * wv[k] : 0.0;
            part = wave_allsum_f64(part);
            if (lane == 0) wsq[s] = part;
        }
        if (wave == FR_WAVES - 1) {
            double part = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) part += lane + k * BSC_WAVE < P ? rv[k] : 0.0;
            part = wave_allsum_f64(part);
            if (lane == 0) rho_sum = part;
        }
    }
    const double phiv = exp(tauv);
    if (tid < n_g) gs[gr][gsmp] = gi < D ? a.scale * Gv - a.prec * Wv : a.scale * Tv + a.a0 - a.b0 * phiv;
    __syncthreads();

    // f_s, by the thread that holds tau_s (the tau row is row1 of workgroup 0), into the slot of |w_s|^2
    if (tau_wg && tid < n_g && gi == D)
        wsq[gsmp] = a.scale * ellv + a.c0 - 0.5 * a.prec * wsq[gsmp] + a.a0 * tauv - a.b0 * phiv;

    fr_grad_adam(rp, P, P, S, gs, a.lam_in, a.lam_out, a.m1, a.m2, a.grad, a.eps, a.adam, Lnew, mu_new);
    __syncthreads();
    if (tau_wg && tid == 0) {
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += wsq[s];
        a.elbo[0] = fsum * inv_S + rho_sum + 0.5 * (double)P * (1.0 + BSC_LOG_2PI);
    }
    if (!a.eps_next) return;

    fr_next_draw(rp, P, S, a.eps_next, Lnew, mu_new, [&](int s, int i, double z) {
        if (i < D) a.W_next[(int64_t)s * D + i] = (float)z;
        else a.logscalar_next[s] = (float)z;
    });
}

}  // namespace

extern "C" {

int bsc_glm_scalar_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                                   double* m2, const double* eps, const float* W, const float* logscalar, int32_t D,
                                   int32_t S, double scale, double prior_precision, double a0, double b0, int64_t t,
                                   double lr, double beta1, double beta2, double adam_eps, uint64_t seed,
                                   uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                                   float* logscalar_next, double* elbo, double* grad) {
    const char* who = "bsc_glm_scalar_fullrank_update";
    BSC_CHECK_CTX(ctx);
    int rc = fr_check_state(who, "ell | G | T", stats,
                            lam_in && lam_out && m1 && m2 && eps && W && logscalar && elbo && grad, lam_in, lam_out, D,
                            SF_MAX_D, S, t);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(prior_precision > 0.0, "%s: prior_precision=%g must be positive", who, prior_precision);
    BSC_REQUIRE(a0 > 0.0 && b0 > 0.0, "%s: a0=%g b0=%g must be positive", who, a0, b0);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, logscalar, eps_next, W_next, logscalar_next, D, S, seed,
                         next_step, eps_next_ready);
    if (rc != BSC_OK) return rc;
    GlmScalarFullArgs a;
    a.stats = stats;
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.logscalar = logscalar;
    a.eps_next = eps_next; a.W_next = W_next; a.logscalar_next = logscalar_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) + a0 * log(b0) - lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(glm_scalar_fullrank_update_kernel, dim3((D + 2) / 2), dim3(FR_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
