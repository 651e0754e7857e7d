// Full-covariance Gaussian guide for the GLM SVI path (Bernoulli-logit and Poisson-log regression): the finish of one
// update.
//
// q(w) = N(mu, L L^T) over w in R^D (no scalar latent: P = D), L lower-triangular with L_ii = e^{rho_i}.
// lam = [mu (D) | L packed row-major, lower triangle incl. the diagonal (D(D+1)/2)]; row i starts at D + i(i+1)/2 and
// its diagonal slot holds rho_i: csrc/bsc_blr_full.hip's layout with P = D.  The data pass (bsc_glm_data_pass,
// unchanged) gives ell_s and G_s for the draws W_s; everything here is parameter-sized float64 work (Kucukelbir et
// al., full-rank ADVI) under the prior w ~ N(0, I / tau):
//     g_s         = scale G_s - tau W_s                  (W_s: the float32-rounded draw the pass read)
//     d / d mu    = mean_s g_s
//     d / d L_ij  = mean_s g_si eps_sj                   (j < i)
//     d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
//     ELBO        = mean_s [scale ell_s - tau/2 |w_s|^2] + D/2 log(tau / 2 pi) + sum_i rho_i + D/2 (1 + log 2 pi)
// then Adam ascent on every entry (bsc_adam_ascent) and the next draw w'_s = mu' + L' eps'_s.
//
// Rows of L are independent (g_si needs column i of G and W only), so workgroup k owns rows k and D-1-k (k + 1 and
// D - k entries: D + 1 together, plus two of mu): (D + 1) / 2 workgroups of equal work.  D is a multiple of 4, so no
// workgroup is left with a single middle row; the code below is written for that case all the same.  Workgroup 0 also
// owns |w_s|^2, sum rho and the ELBO.  Each workgroup forms its rows of the next draw from its own rows of L'.  Every
// sum runs in a fixed order, no atomics, no inter-workgroup communication: the result is the same bytes run to run.
// The caller double-buffers lam and the draws.  Small and latency-bound: a handful of dependent memory round trips per
// workgroup, and short on purpose -- the finish starts instruction-cache cold behind the pass (NOTES section 4).
#include "bsc_fullrank.h"

// as the regression full-rank finish (csrc/bsc_blr_full.hip): no contraction into FMAs.  With a diagonal L this is the
// mean-field finish's arithmetic (csrc/bsc_glm.hip) but for the two moment updates of Adam, which glm_update_kernel
// fuses (bsc_adam_ascent<true>, csrc/bsc_regress.h): the two finishes agree to rtol 1e-12, not bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int GF_MAX_D = 256;

struct GlmFullArgs {
    const double* stats;     // [ell (S) | G (S*D)]
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;       // [S, D + 1] (bsc_blr_noise's layout; column D is not read)
    const float* W;
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    double* elbo;
    double* grad;            // lam's layout
    int D, S;
    double scale, tau, c0;   // c0 = D/2 log(tau / 2 pi) + D/2 (1 + log 2 pi)
    bsc_adam adam;
};

__global__ __launch_bounds__(FR_BLOCK) void glm_fullrank_update_kernel(GlmFullArgs a) {
    __shared__ double wsq[FR_MAX_S];
    __shared__ double gs[2][FR_MAX_S];     // g_{s,i} of the two rows
    __shared__ double Lnew[2][GF_MAX_D];   // the rows of L' (diagonal as e^{rho'})
    __shared__ double mu_new[2];
    __shared__ double rho_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S, E = D + 1;   // E: row stride of the noise layout
    const fr_rows rp = fr_row_pair(blockIdx.x, D);
    const bool elbo_wg = blockIdx.x == 0;
    const double inv_S = 1.0 / (double)S;

    // ---- g_{s,i} for the rows of this workgroup (and, in workgroup 0, |w_s|^2 and sum rho) ----
    for (int idx = tid; idx < rp.n_rows * S; idx += FR_BLOCK) {
        const int r = idx / S, s = idx - r * S, i = r ? rp.row1 : rp.row0;
        const double wv = (double)a.W[(int64_t)s * D + i];
        gs[r][s] = a.scale * a.stats[S + (int64_t)s * D + i] - a.tau * wv;
    }
    if (elbo_wg) {
        for (int s = wave; s < S; s += FR_WAVES) {
            double part = 0.0;
            for (int d = lane; d < D; d += BSC_WAVE) {
                const double wv = (double)a.W[(int64_t)s * D + d];
                part += wv * wv;
            }
            part = wave_allsum_f64(part);
            if (lane == 0) wsq[s] = part;
        }
        if (wave == FR_WAVES - 1) {
            double part = 0.0;
            for (int i = lane; i < D; i += BSC_WAVE) part += a.lam_in[D + i * (i + 1) / 2 + i];
            part = wave_allsum_f64(part);
            if (lane == 0) rho_sum = part;
        }
    }
    __syncthreads();

    fr_grad_adam(rp, D, E, S, gs, a.lam_in, a.lam_out, a.m1, a.m2, a.grad, a.eps, a.adam, Lnew, mu_new);
    if (elbo_wg && tid == 0) {
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += a.scale * a.stats[s] - 0.5 * a.tau * wsq[s];
        a.elbo[0] = fsum * inv_S + a.c0 + rho_sum;
    }
    if (!a.eps_next) return;
    __syncthreads();

    fr_next_draw(rp, E, S, a.eps_next, Lnew, mu_new,
                 [&](int s, int i, double z) { a.W_next[(int64_t)s * D + i] = (float)z; });
}

}  // namespace

extern "C" {

int bsc_glm_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, int32_t D, int32_t S, double scale,
                            double prior_precision, int64_t t, double lr, double beta1, double beta2, double adam_eps,
                            uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready, float* W_next,
                            double* elbo, double* grad) {
    const char* who = "bsc_glm_fullrank_update";
    BSC_CHECK_CTX(ctx);
    int rc = fr_check_state(who, "ell | G", stats, lam_in && lam_out && m1 && m2 && eps && W && elbo && grad, lam_in,
                            lam_out, D, GF_MAX_D, S, t);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(prior_precision > 0.0, "%s: prior_precision=%g must be positive", who, prior_precision);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    rc = next_draw_noise(ctx, who, /*has_extra=*/false, eps, W, nullptr, eps_next, W_next, nullptr, D, S, seed,
                         next_step, eps_next_ready);
    if (rc != BSC_OK) return rc;
    GlmFullArgs a;
    a.stats = stats;
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W;
    a.eps_next = eps_next; a.W_next = W_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.tau = prior_precision;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) + 0.5 * (double)D * (1.0 + BSC_LOG_2PI);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(glm_fullrank_update_kernel, dim3((D + 1) / 2), dim3(FR_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
