// Negative-binomial regression with a learned dispersion on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies
// with the dispersion flag on, their slab reduction, the finish for the latent z = [w (D) | tau], and the predictive
// (csrc/bsc_predict_pass.h's body with its fourth family).
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
#include "bsc_glm_pass.h"
#include "bsc_predict_pass.h"

namespace {

constexpr int MAX_S = 64;

// ---- the pass ---------------------------------------------------------------------------------------------------------

template <bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_nb_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, const float* __restrict__ logphi, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_body<GLM_NEGBIN, FULL, true, false, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, nullptr, logphi);
}

__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_nb_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, const float* __restrict__ logphi, int S,
    float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GLM_NEGBIN, true, false, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, nullptr, logphi);
}

__global__ __launch_bounds__(RED_BLOCK) void glm_nb_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                       int D, int S, int s_base,
                                                                       double* __restrict__ ell, double* __restrict__ G,
                                                                       double* __restrict__ T) {
    regress_slab_reduce<NB_SLAB_STRIDE>(slab, n_blocks, D, S, s_base, ell, G, T);
}

// ---- the finish -------------------------------------------------------------------------------------------------------

struct NbArgs {
    const double* stats;     // [ell (S) | G (S D) | T (S)]
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;       // [S, D + 1]: columns 0 .. D - 1 stream 0, column D (tau) stream 1
    const float* W;          // [S, D]
    const float* logphi;     // [S]
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    float* logphi_next;
    double* scal;            // [g_tau (64) | f (64) | sum rho]
    double* elbo;
    double* grad;
    int D, S;
    double scale, prec, a0, b0;
    double c0;               // the terms of log p(z) free of z: D/2 log(prec / 2 pi) + a0 log b0 - lnGamma(a0)
    bsc_adam adam;
};

constexpr int NB_BLOCK = 256;
constexpr int NB_WAVES = NB_BLOCK / BSC_WAVE;

// the block's sum of one value per thread: waves in wave order
__device__ __forceinline__ double nb_block_sum(double v, double* red) {
    v = wave_allsum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int k = 1; k < NB_WAVES; ++k) t += red[k];
    __syncthreads();
    return t;
}

// Workgroup s < S: |w_s|^2, g_tau and f_s = scale ell_s + log p(z_s) with tau_s the float32 value the pass read;
// workgroup S: sum rho.
__global__ __launch_bounds__(NB_BLOCK) void glm_nb_scalars_kernel(NbArgs a) {
    __shared__ double red[NB_WAVES];
    const int tid = threadIdx.x;
    const int D = a.D, S = a.S, P = D + 1;
    const int s = (int)blockIdx.x;
    if (s == S) {
        double part = 0.0;
        for (int i = tid; i < P; i += NB_BLOCK) part += a.lam_in[P + i];
        const double t = nb_block_sum(part, red);
        if (tid == 0) a.scal[2 * MAX_S] = t;
        return;
    }
    double pw = 0.0;
    for (int d = tid; d < D; d += NB_BLOCK) {
        const double wv = (double)a.W[(int64_t)s * D + d];
        pw += wv * wv;
    }
    const double wsq = nb_block_sum(pw, red);
    if (tid == 0) {
        const double tau = (double)a.logphi[s];
        const double phi = exp(tau);
        const double T = a.stats[S + (int64_t)S * D + s];
        a.scal[s] = a.scale * T + a.a0 - a.b0 * phi;
        a.scal[MAX_S + s] = a.scale * a.stats[s] + a.c0 - 0.5 * a.prec * wsq + a.a0 * tau - a.b0 * phi;
    }
}

// One thread per coordinate i of z: gradient over the draws in draw order, Adam, the next draws.
__global__ __launch_bounds__(NB_BLOCK) void glm_nb_coord_kernel(NbArgs a) {
    const int D = a.D, S = a.S, P = D + 1;
    const int i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= P) return;
    const double* G = a.stats + S;
    double gm = 0.0, gr = 0.0;
    for (int s = 0; s < S; ++s) {
        const double g = i < D ? a.scale * G[(int64_t)s * D + i] - a.prec * (double)a.W[(int64_t)s * D + i] : a.scal[s];
        gm += g;
        gr += g * a.eps[(int64_t)s * P + i];
    }
    const double inv_S = 1.0 / (double)S;
    const double p_m = a.lam_in[i], p_rho = a.lam_in[P + i];
    const double g_m = gm * inv_S;
    const double g_r = gr * inv_S * exp(p_rho) + 1.0;
    a.grad[i] = g_m;
    a.grad[P + i] = g_r;
    double q1 = a.m1[i], q2 = a.m2[i];
    const double nm = bsc_adam_ascent(p_m, g_m, q1, q2, a.adam);
    a.m1[i] = q1; a.m2[i] = q2;
    q1 = a.m1[P + i]; q2 = a.m2[P + i];
    const double nr = bsc_adam_ascent(p_rho, g_r, q1, q2, a.adam);
    a.m1[P + i] = q1; a.m2[P + i] = q2;
    a.lam_out[i] = nm;
    a.lam_out[P + i] = nr;
    if (i == P - 1) {
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += a.scal[MAX_S + s];
        a.elbo[0] = fsum * inv_S + a.scal[2 * MAX_S] + 0.5 * (double)P * (1.0 + BSC_LOG_2PI);
    }
    if (!a.eps_next) return;
    const double sd = exp(nr);
    if (i < D) {
        for (int s = 0; s < S; ++s) a.W_next[(int64_t)s * D + i] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
    } else {
        for (int s = 0; s < S; ++s) a.logphi_next[s] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
    }
}

// ---- the predictive ---------------------------------------------------------------------------------------------------

// FULL: D == 256.  offset may be null.
template <int NC, bool FULL>
__global__ __launch_bounds__(P_BLOCK, 2) void predict_nb_kernel(PredictArgs a, const float* __restrict__ offset) {
    predict_body<PREDICT_NEGBIN, NC, FULL, true>(a, offset);
}

__global__ __launch_bounds__(BSC_WAVE) void predict_nb_sum_kernel(const double* __restrict__ partial, int n,
                                                                  double* __restrict__ out) {
    block_partial_sum(partial, n, out);
}

template <int NC>
void launch_predict_nb_nc(bsc_ctx* ctx, const PredictArgs& a, const float* offset, int n_blocks) {
    const dim3 grid(n_blocks), block(P_BLOCK);
    if (a.D == WCOLS) hipLaunchKernelGGL((predict_nb_kernel<NC, true>), grid, block, 0, ctx->stream, a, offset);
    else hipLaunchKernelGGL((predict_nb_kernel<NC, false>), grid, block, 0, ctx->stream, a, offset);
}

#define NB_UNSUPPORTED(cond, ...)                                         \
    do {                                                                  \
        if (!(cond)) return bsc_fail(BSC_ERR_UNSUPPORTED, __VA_ARGS__);   \
    } while (0)

}  // namespace

extern "C" {

int bsc_glm_nb_data_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset,
                         const float* weight, int64_t B, int32_t D, const float* W, const float* logphi, int32_t S,
                         double* ell, double* G, double* T) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_nb_data_pass";
    const int rc0 = check_glm_obs_args(who, BSC_GLM_LOGISTIC, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc0 != BSC_OK) return rc0;
    BSC_REQUIRE(logphi, "%s: logphi is null", who);
    BSC_REQUIRE((((uintptr_t)logphi) & 3) == 0, "%s: logphi must be 4-byte aligned", who);
    BSC_REQUIRE(ell && G && T, "%s: null output", who);

    const int rows = pass_rows(D, y, offset, weight);
    const PassGrid g = pass_grid(ctx, B, rows);
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * NB_SLAB_STRIDE * sizeof(float), &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    const dim3 grid(g.n_blocks), block(PASS_BLOCK);
    const dim3 rgrid((NB_SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    for (int s0 = 0; s0 < S; s0 += SG) {   // eight draws per launch, each with its chunk of logphi
        const int sg = S - s0 < SG ? S - s0 : SG;
        const float* Ws = W + (int64_t)s0 * D;
        {
            bsc_prof_scope prof(ctx);  // times the pass kernel alone
            if (rows == MT_ROWS)
                hipLaunchKernelGGL(glm_nb_pass_mfma_kernel, grid, block, 0, ctx->stream, X, ldx, y, offset, weight,
                                   B, Ws, logphi + s0, sg, slab, g.n_iter);
            else if (D == GCOLS)
                hipLaunchKernelGGL((glm_nb_pass_kernel<true>), grid, block, 0, ctx->stream, X, ldx, y, offset, weight, B,
                                   (int)D, Ws, logphi + s0, sg, slab, g.n_iter);
            else
                hipLaunchKernelGGL((glm_nb_pass_kernel<false>), grid, block, 0, ctx->stream, X, ldx, y, offset, weight,
                                   B, (int)D, Ws, logphi + s0, sg, slab, g.n_iter);
        }
        BSC_LAUNCH_CHECK();
        hipLaunchKernelGGL(glm_nb_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, (const float*)slab,
                           g.n_blocks, (int)D, (int)S, s0, ell, G, T);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

int bsc_glm_nb_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                      const double* eps, const float* W, const float* logphi, int32_t D, int32_t S, double scale,
                      double prior_precision, double a0, double b0, int64_t t, double lr, double beta1, double beta2,
                      double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                      float* W_next, float* logphi_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_nb_update";
    BSC_REQUIRE(stats, "%s: stats is null (pending pass partials are not read: pass [ell | G | T])", who);
    BSC_REQUIRE(lam_in && lam_out && m1 && m2 && eps && W && logphi && elbo && grad, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D > 0 && S >= 1 && S <= MAX_S, "%s: D=%d S=%d (S<=%d)", who, D, S, MAX_S);
    BSC_REQUIRE(prior_precision > 0.0, "%s: prior_precision=%g must be positive", who, prior_precision);
    BSC_REQUIRE(a0 > 0.0 && b0 > 0.0, "%s: a0=%g b0=%g must be positive", who, a0, b0);
    BSC_REQUIRE(scale > 0.0, "%s: scale=%g must be positive", who, scale);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    BSC_REQUIRE((eps_next && W_next && logphi_next) || (!eps_next && !W_next && !logphi_next),
                "%s: next-draw buffers must be all set or all null", who);
    BSC_REQUIRE(!eps_next || (eps_next != eps && W_next != W && logphi_next != logphi),
                "%s: next-draw buffers must not alias the current draws", who);
    const int P = D + 1;
    void* ws = nullptr;
    int rc = bsc_workspace(ctx, (2 * MAX_S + 8) * sizeof(double), &ws);
    if (rc != BSC_OK) return rc;
    if (eps_next && !eps_next_ready) {   // the noise of next_step first (off the default path: drivers draw ahead)
        rc = bsc_blr_noise(ctx, D, S, seed, next_step, 1, eps_next);
        if (rc != BSC_OK) return rc;
    }
    NbArgs a;
    a.stats = stats; a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.logphi = logphi; a.eps_next = eps_next; a.W_next = W_next; a.logphi_next = logphi_next;
    a.scal = (double*)ws; a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) + a0 * log(b0) - lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    ctx->slab_rows = 0;   // the workspace is this finish's now
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish, timed apart from the pass
        hipLaunchKernelGGL(glm_nb_scalars_kernel, dim3(S + 1), dim3(NB_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(glm_nb_coord_kernel, dim3((P + NB_BLOCK - 1) / NB_BLOCK), dim3(NB_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_nb_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, const float* offset, int64_t B,
                        int32_t D, const float* W, const float* logphi, int32_t S, float* mean, float* var, float* lpd,
                        double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_nb_predict_pass";
    BSC_REQUIRE(B >= 0, "%s: B=%lld", who, (long long)B);
    BSC_REQUIRE((X || B == 0) && W, "%s: null pointer", who);
    BSC_REQUIRE(logphi, "%s: logphi is null", who);
    BSC_REQUIRE(mean || var || lpd || lpd_sum, "%s: no output requested", who);
    BSC_REQUIRE(y || B == 0 || (!lpd && !lpd_sum), "%s: lpd and lpd_sum need y", who);
    BSC_REQUIRE((((uintptr_t)offset) & 3) == 0 && (((uintptr_t)logphi) & 3) == 0,
                "%s: offset and logphi must be 4-byte aligned", who);
    NB_UNSUPPORTED(D > 0 && D <= WCOLS && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, WCOLS);
    NB_UNSUPPORTED(S >= 1 && S <= P_MAX_S, "%s: S=%d must be in [1,%d]", who, S, P_MAX_S);
    NB_UNSUPPORTED(ldx >= D && ldx % 4 == 0 && ldx < ((int64_t)1 << 26), "%s: ldx=%lld must be >= D, %% 4 == 0 and < 2^26",
                   who, (long long)ldx);
    NB_UNSUPPORTED(((uintptr_t)X & 15) == 0 && ((uintptr_t)W & 15) == 0, "%s: X and W must be 16-byte aligned", who);
    if (B == 0) {
        if (lpd_sum) BSC_HIP(hipMemsetAsync(lpd_sum, 0, sizeof(double), ctx->stream));
        return BSC_OK;
    }
    // one workgroup per CU; every wave runs the same number of tiles (bsc_predict_pass's grid)
    const int64_t n_tiles = (B + T_ROWS - 1) / T_ROWS;
    const int64_t max_waves = (int64_t)P_WAVES * ctx->cu_count;
    const int64_t n_iter = (n_tiles + max_waves - 1) / max_waves;
    NB_UNSUPPORTED(n_iter < ((int64_t)1 << 30), "%s: B=%lld is too large", who, (long long)B);
    const int64_t waves = (n_tiles + n_iter - 1) / n_iter;
    const int n_blocks = (int)((waves + P_WAVES - 1) / P_WAVES);

    PredictArgs a;
    a.X = X; a.ldx = ldx; a.y = y; a.B = B; a.W = W; a.logvar = logphi;
    a.mean = mean; a.var = var; a.lpd = lpd; a.partial = nullptr;
    a.D = D; a.S = S;
    a.n_iter = (int)n_iter;
    a.n_strips = D > STRIP ? 2 : 1;
    a.kw = D > STRIP ? STRIP / 4 : ((D + 7) / 8) * 2;
    a.do_lp = (y && (lpd || lpd_sum)) ? 1 : 0;
    if (lpd_sum) {
        void* ws = nullptr;
        const int rc = bsc_workspace(ctx, (size_t)n_blocks * sizeof(double), &ws);
        if (rc != BSC_OK) return rc;
        ctx->slab_rows = 0;   // pass partials that were pending in the workspace are gone
        a.partial = (double*)ws;
    }
    {
        bsc_prof_scope prof(ctx);
        if (S <= 16) launch_predict_nb_nc<1>(ctx, a, offset, n_blocks);
        else if (S <= 32) launch_predict_nb_nc<2>(ctx, a, offset, n_blocks);
        else launch_predict_nb_nc<4>(ctx, a, offset, n_blocks);
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(predict_nb_sum_kernel, dim3(1), dim3(BSC_WAVE), 0, ctx->stream, (const double*)a.partial,
                           n_blocks, lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
