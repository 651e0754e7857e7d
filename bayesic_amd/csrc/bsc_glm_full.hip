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
// then Adam ascent on every entry (adam_ascent_one's arithmetic) and the next draw w'_s = mu' + L' eps'_s.
//
// Rows of L are independent (g_si needs column i of G and W only), so workgroup k owns rows k and D-1-k (k + 1 and
// D - k entries: D + 1 together, plus two of mu): (D + 1) / 2 workgroups of equal work.  D is a multiple of 4, so no
// workgroup is left with a single middle row; the code below is written for that case all the same.  Workgroup 0 also
// owns |w_s|^2, sum rho and the ELBO.  Each workgroup forms its rows of the next draw from its own rows of L'.  Every
// sum runs in a fixed order, no atomics, no inter-workgroup communication: the result is the same bytes run to run.
// The caller double-buffers lam and the draws.  Small and latency-bound: a handful of dependent memory round trips per
// workgroup, and short on purpose -- the finish starts instruction-cache cold behind the pass (NOTES section 4).
#include "bsc_common.h"

// as the mean-field finish (csrc/bsc_glm.hip) and the regression full-rank finish (csrc/bsc_blr_full.hip): no
// contraction into FMAs, so that with a diagonal L the finishes do the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int GF_BLOCK = 256;
constexpr int GF_WAVES = GF_BLOCK / BSC_WAVE;
constexpr int GF_MAX_S = 64;
constexpr int GF_MAX_D = 256;
constexpr double GF_LOG_2PI = 1.8378770664093454835606594728112;

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
    double lr, beta1, beta2, adam_eps, corr1, corr2;
};

// adam_ascent_one (csrc/bsc_glm.hip) / fr_adam (csrc/bsc_blr_full.hip), the same arithmetic
__device__ __forceinline__ double gf_adam(double lam, double g, double& m1, double& m2, const GlmFullArgs& a) {
    const double na = a.beta1 * m1 + (1.0 - a.beta1) * g;
    const double nb = a.beta2 * m2 + (1.0 - a.beta2) * g * g;
    m1 = na;
    m2 = nb;
    const double mhat = na / a.corr1;
    const double vhat = nb / a.corr2;
    return lam + a.lr * mhat / (sqrt(vhat) + a.adam_eps);
}

__global__ __launch_bounds__(GF_BLOCK) void glm_fullrank_update_kernel(GlmFullArgs a) {
    __shared__ double wsq[GF_MAX_S];
    __shared__ double gs[2][GF_MAX_S];     // g_{s,i} of the two rows
    __shared__ double Lnew[2][GF_MAX_D];   // the rows of L' (diagonal as e^{rho'})
    __shared__ double mu_new[2];
    __shared__ double rho_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S, E = D + 1;   // E: row stride of the noise layout
    const int k = blockIdx.x;
    const int row0 = k, row1 = D - 1 - k;  // row1 >= row0
    const int n_rows = row0 == row1 ? 1 : 2;
    const bool elbo_wg = k == 0;
    const double inv_S = 1.0 / (double)S;

    // ---- g_{s,i} for the rows of this workgroup (and, in workgroup 0, |w_s|^2 and sum rho) ----
    for (int idx = tid; idx < n_rows * S; idx += GF_BLOCK) {
        const int r = idx / S, s = idx - r * S, i = r ? row1 : row0;
        const double wv = (double)a.W[(int64_t)s * D + i];
        gs[r][s] = a.scale * a.stats[S + (int64_t)s * D + i] - a.tau * wv;
    }
    if (elbo_wg) {
        for (int s = wave; s < S; s += GF_WAVES) {
            double part = 0.0;
            for (int d = lane; d < D; d += BSC_WAVE) {
                const double wv = (double)a.W[(int64_t)s * D + d];
                part += wv * wv;
            }
            part = wave_allsum_f64(part);
            if (lane == 0) wsq[s] = part;
        }
        if (wave == GF_WAVES - 1) {
            double part = 0.0;
            for (int i = lane; i < D; i += BSC_WAVE) part += a.lam_in[D + i * (i + 1) / 2 + i];
            part = wave_allsum_f64(part);
            if (lane == 0) rho_sum = part;
        }
    }
    __syncthreads();

    // ---- gradient + Adam: one entry per thread; item j = -1 is mu_i, j = 0..i the row's entries of L ----
    const int n0 = row0 + 2;
    const int n_items = n0 + (n_rows == 2 ? row1 + 2 : 0);
    for (int it = tid; it < n_items; it += GF_BLOCK) {
        const int r = it < n0 ? 0 : 1;
        const int i = r ? row1 : row0;
        const int j = (r == 0 ? it : it - n0) - 1;
        const int64_t off = j < 0 ? (int64_t)i : (int64_t)D + (int64_t)i * (i + 1) / 2 + j;
        const double p = a.lam_in[off];
        double m1 = a.m1[off], m2 = a.m2[off];
        double acc = 0.0;
        if (j < 0) {
            for (int s = 0; s < S; ++s) acc += gs[r][s];
        } else {
            for (int s = 0; s < S; ++s) acc += gs[r][s] * a.eps[(int64_t)s * E + j];
        }
        double g = acc * inv_S;
        if (j == i) g = g * exp(p) + 1.0;
        a.grad[off] = g;
        const double np = gf_adam(p, g, m1, m2, a);
        a.m1[off] = m1;
        a.m2[off] = m2;
        a.lam_out[off] = np;
        if (j < 0) mu_new[r] = np;
        else Lnew[r][j] = j == i ? exp(np) : np;
    }
    if (elbo_wg && tid == 0) {
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += a.scale * a.stats[s] - 0.5 * a.tau * wsq[s];
        a.elbo[0] = fsum * inv_S + a.c0 + rho_sum;
    }
    if (!a.eps_next) return;
    __syncthreads();

    // ---- next draw of these rows: w'_{s,i} = mu'_i + sum_{j<=i} L'_ij eps'_sj (a wave per sample, both rows at once) ----
    for (int s = wave; s < S; s += GF_WAVES) {
        const double* e = a.eps_next + (int64_t)s * E;
        double z0 = 0.0, z1 = 0.0;
        for (int j = lane; j <= row1; j += BSC_WAVE) {
            const double ev = e[j];
            if (j <= row0) z0 += Lnew[0][j] * ev;
            z1 += Lnew[n_rows - 1][j] * ev;
        }
        z0 = wave_allsum_f64(z0);
        z1 = wave_allsum_f64(z1);
        if (lane == 0) {
            a.W_next[(int64_t)s * D + row0] = (float)(mu_new[0] + z0);
            if (n_rows == 2) a.W_next[(int64_t)s * D + row1] = (float)(mu_new[1] + z1);
        }
    }
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
    BSC_REQUIRE(stats, "%s: stats must be the [ell | G] of the data pass (pending partials are not read)", who);
    BSC_REQUIRE(lam_in && lam_out && m1 && m2 && eps && W && elbo && grad, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D >= 4 && D <= GF_MAX_D && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, GF_MAX_D);
    BSC_REQUIRE(S >= 1 && S <= GF_MAX_S, "%s: S=%d must be in [1,%d]", who, S, GF_MAX_S);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    BSC_REQUIRE(prior_precision > 0.0, "%s: prior_precision=%g must be positive", who, prior_precision);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    BSC_REQUIRE((eps_next && W_next) || (!eps_next && !W_next), "%s: next-draw buffers must be both set or both null",
                who);
    BSC_REQUIRE(!eps_next || (eps_next != eps && W_next != W), "%s: next-draw buffers must not alias the current draws",
                who);
    if (eps_next && !eps_next_ready) {   // the next step's noise first (bsc_blr_noise's layout), then the finish
        const int rc = bsc_blr_noise(ctx, D, S, seed, next_step, 1, eps_next);
        if (rc != BSC_OK) return rc;
    }
    GlmFullArgs a;
    a.stats = stats;
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W;
    a.eps_next = eps_next; a.W_next = W_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.tau = prior_precision;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - GF_LOG_2PI) + 0.5 * (double)D * (1.0 + GF_LOG_2PI);
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.adam_eps = adam_eps;
    a.corr1 = 1.0 - pow(beta1, (double)t);
    a.corr2 = 1.0 - pow(beta2, (double)t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(glm_fullrank_update_kernel, dim3((D + 1) / 2), dim3(GF_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
