// Full-covariance Gaussian guide for the regression SVI path (BASELINE config 2): the finish of one update.
//
// q(z) = N(mu, L L^T) over z = [w (D) | xi], P = D + 1, L lower-triangular with L_ii = e^{rho_i}.
// lam = [mu (P) | L packed row-major, lower triangle incl. the diagonal (P(P+1)/2)]; row i starts at
// P + i(i+1)/2 and its diagonal slot holds rho_i.  The data pass (bsc_blr_data_pass[_sweep], unchanged) gives
// Q_s and G_s for the draws W_s; everything here is parameter-sized float64 work (Kucukelbir et al., full-rank ADVI):
//     g_s         = d f / d z at z_s = mu + L eps_s      (w part: e^{-xi_s} (s_q G_s - k_w W_s), W_s float32-rounded)
//     d / d mu    = mean_s g_s
//     d / d L_ij  = mean_s g_si eps_sj                   (j < i)
//     d / d rho_i = mean_s g_si eps_si e^{rho_i} + 1
//     ELBO        = mean_s f_s + sum_i rho_i + P/2 (1 + log 2 pi)
// then Adam ascent on every entry (bsc_adam_ascent) and the next draw z'_s = mu' + L' eps'_s.
//
// Rows of L are independent once the per-sample scalars e^{-xi_s} (and, for the xi row, |w_s|^2 and Q_s) are known, so
// workgroup k owns rows k and P-1-k (i + 1 and P - i entries: P + 1 together; P = D + 1 is odd, so the middle row
// (P-1)/2 is a workgroup of its own): (P + 1) / 2 workgroups of equal work.  Workgroup 0 owns the xi row and writes
// the ELBO.  Each workgroup forms its rows of the next draw from its own rows of L'.  Every sum runs in a fixed order,
// no atomics, no inter-workgroup communication: the result is the same bytes run to run.  The caller double-buffers
// lam and the draws.  Small and latency-bound: a handful of dependent memory round trips per workgroup.
#include "bsc_fullrank.h"

// as the mean-field finish (csrc/bsc_blr.hip): no contraction into FMAs, so that with a diagonal L the two finishes do
// the same arithmetic
#pragma clang fp contract(off)

namespace {

constexpr int FR_MAX_P = 257;

struct FullArgs {
    const double* stats;   // [Q (S) | G (S*D)]
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;     // [S, P]: stream 0 for w, stream 1 for xi (bsc_blr_noise)
    const float* W;
    const double* xi;
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    double* xi_next;
    double* elbo;
    double* grad;          // lam's layout
    int D, S;
    double c0, c_xi, s_q, k_w, beta;
    bsc_adam adam;
};

__global__ __launch_bounds__(FR_BLOCK) void blr_fullrank_update_kernel(FullArgs a) {
    __shared__ double e_inv[FR_MAX_S];
    __shared__ double wsq[FR_MAX_S];
    __shared__ double gs[2][FR_MAX_S];     // g_{s,i} of the two rows
    __shared__ double ft[FR_MAX_S];        // f_s (workgroup 0)
    __shared__ double Lnew[2][FR_MAX_P];   // the rows of L' (diagonal as e^{rho'})
    __shared__ double mu_new[2];
    __shared__ double rho_sum;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S, P = D + 1;
    const fr_rows rp = fr_row_pair(blockIdx.x, P);
    const bool xi_wg = blockIdx.x == 0;    // owns row P-1 (xi) and the ELBO
    const double inv_S = 1.0 / (double)S;

    // ---- per-sample scalars (and, in workgroup 0, |w_s|^2 and sum rho) ----
    if (tid < S) e_inv[tid] = exp(-a.xi[tid]);
    if (xi_wg) {
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
            for (int i = lane; i < P; i += BSC_WAVE) part += a.lam_in[P + i * (i + 1) / 2 + i];
            part = wave_allsum_f64(part);
            if (lane == 0) rho_sum = part;
        }
    }
    __syncthreads();

    // ---- g_{s,i} for the rows of this workgroup ----
    for (int idx = tid; idx < rp.n_rows * S; idx += FR_BLOCK) {
        const int r = idx / S, s = idx - r * S, i = r ? rp.row1 : rp.row0;
        const double e = e_inv[s];
        if (i < D) {
            const double wv = (double)a.W[(int64_t)s * D + i];
            gs[r][s] = e * (a.s_q * a.stats[S + (int64_t)s * D + i] - a.k_w * wv);
        } else {
            const double x = a.xi[s];
            const double inner = 0.5 * a.s_q * a.stats[s] + 0.5 * a.k_w * wsq[s] + a.beta;
            gs[r][s] = a.c_xi + e * inner;
            ft[s] = a.c0 + a.c_xi * x - e * inner;
        }
    }
    __syncthreads();

    fr_grad_adam(rp, P, P, S, gs, a.lam_in, a.lam_out, a.m1, a.m2, a.grad, a.eps, a.adam, Lnew, mu_new);
    if (xi_wg && tid == 0) {
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += ft[s];
        a.elbo[0] = fsum * inv_S + rho_sum + 0.5 * (double)P * (1.0 + BSC_LOG_2PI);
    }
    if (!a.eps_next) return;
    __syncthreads();

    fr_next_draw(rp, P, S, a.eps_next, Lnew, mu_new, [&](int s, int i, double z) {
        if (i < D) a.W_next[(int64_t)s * D + i] = (float)z;
        else a.xi_next[s] = z;
    });
}

}  // namespace

extern "C" {

int bsc_blr_fullrank_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                            double* m2, const double* eps, const float* W, const double* xi, int32_t D, int32_t S,
                            double c0, double c_xi, double s_q, double k_w, double beta, int64_t t, double lr,
                            double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                            double* eps_next, int32_t eps_next_ready, float* W_next, double* xi_next, double* elbo,
                            double* grad) {
    const char* who = "bsc_blr_fullrank_update";
    BSC_CHECK_CTX(ctx);
    int rc = fr_check_state(who, "Q | G", stats, lam_in && lam_out && m1 && m2 && eps && W && xi && elbo && grad, lam_in,
                            lam_out, D, FR_MAX_P - 1, S, t);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(s_q >= 0.0 && k_w >= 0.0, "%s: s_q=%g k_w=%g must not be negative", who, s_q, k_w);
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, xi, eps_next, W_next, xi_next, D, S, seed, next_step,
                         eps_next_ready);
    if (rc != BSC_OK) return rc;
    FullArgs a;
    a.stats = stats;
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.xi = xi;
    a.eps_next = eps_next; a.W_next = W_next; a.xi_next = xi_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.c0 = c0; a.c_xi = c_xi; a.s_q = s_q; a.k_w = k_w; a.beta = beta;
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(blr_fullrank_update_kernel, dim3((D + 2) / 2), dim3(FR_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
