// Reparameterised SVI for canonical-link GLMs: Bernoulli-logit and Poisson-log regression.
//
// ABSENT in the reference: README.md:51 (reparameterisation trick, refs [10][11][12]) and README.md:69-79
// (mini-batch SVI) on the likelihood split of bayesic/distribution/base.py:47-69, for the two non-conjugate
// likelihoods people use VI for.  With l_ns = x_n . w_s the data-sized work of one update is
//     ell[s]  = sum_n [y_n l_ns - A(l_ns)]
//     G[s, :] = sum_n (y_n - A'(l_ns)) x_n
// A = softplus (logistic), A = exp (Poisson): the shape of csrc/bsc_blr.hip's pass with another per-row
// function, so the kernels below are that file's -- one read of X[B, D] and y[B] for up to eight draws, the same
// tiles, the same slab of per-workgroup partials ([d * 8 + s] then eight scalars, ell where BLR keeps Q) and
// the same float64 fixed-order reduction (no float atomics: bitwise reproducible).
//
//   D == 256   glm_pass_mfma_kernel: a wave owns 16-row tiles, prefetched through registers (non-temporal
//              buffer loads: X is read once) and parked row-major in the wave's LDS region.  Forward on
//              v_mfma_f32_16x16x4_f32 with W as the B operand: lane (draw = lane % 16, kq = lane / 16) ends with
//              the logits of rows 4 kq .. 4 kq + 3 of its draw in four registers, applies the link to them in
//              place and hands the residuals y - A'(l) to the backward through LDS ([draw][row]).  Backward:
//              the rank-1 updates G[s, :] += r[n, s] x[n, :] on v_mfma_f32_4x4x1_16B_f32 into per-lane
//              accumulators (register i of accumulator (sb, q) = G[4 sb + i][4 lane + q]).
//   otherwise  glm_pass_kernel: 8-row tiles, lane l holds columns 4 l .. 4 l + 3 of every row, the 64 partial
//              dot products of a lane are transposed and summed through the wave's LDS region, the link runs on
//              one (row, draw) per lane, the residuals come back by LDS broadcast.
//
// Rows past the end of the mini-batch read as zeros through the buffer descriptor (no ragged-tail path); their
// logit is 0, so they add nothing to G (x = 0) and are masked out of ell (A(0) != 0).
//
// The bodies live in csrc/bsc_glm_pass.h so that csrc/bsc_glm_obs.hip can instantiate them with per-row offsets and
// weights (bsc_glm_data_pass_obs, bsc_glm_pass_update_obs below); the kernels here are those bodies with that flag off.
#include "bsc_glm_pass.h"

namespace {

constexpr int MAX_S = 64;

// FULL: D == 256.  n_iter: tiles per wave (the same for every wave; tiles past the end read zeros).
template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B, int D,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_body<GlmFamily<LINK>, FULL, false>(X, ldx, y, nullptr, nullptr, B, D, W, S, slab, n_iter);
}

// 16-row tiles, both contractions on the MFMA pipe (D == 256, y 16-byte aligned)
template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, int64_t B,
    const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter) {
    glm_pass_mfma_body<GlmFamily<LINK>, false>(X, ldx, y, nullptr, nullptr, B, W, S, slab, n_iter);
}

// ---- float64 reduction of the slab: blr_slab_reduce_kernel's body, ell where that one writes Q -------------------
__global__ __launch_bounds__(RED_BLOCK) void glm_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks, int D,
                                                                    int S, int s_base, double* __restrict__ ell,
                                                                    double* __restrict__ G) {
    regress_slab_reduce(slab, n_blocks, D, S, s_base, ell, G);
}

// ---- the finish: slab reduce + ELBO + pathwise gradient + Adam + next draw, one launch ----------------------
//
// Grid = ceil(D / 8) column workgroups + 1 scalar workgroup (blr_fused_update_kernel's split).  A column
// workgroup owns 8 columns x 8 draws (one 256-byte run per slab row); the scalar workgroup owns ell, |w_s|^2, the
// entropy term and the ELBO.  lam = [m (D) | rho (D)] is double-buffered by the caller, so no workgroup reads what
// another one writes.
constexpr int FIN_BLOCK = 1024;
constexpr int FIN_WAVES = FIN_BLOCK / BSC_WAVE;

struct GlmArgs {
    const float* slab;       // block partials of the pass kernel, or nullptr
    int n_slab;
    const double* stats;     // [ell (S) | G (S*D)] when slab == nullptr
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;       // [S, D + 1] (bsc_blr_noise's layout; column D is not read)
    const float* W;
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    double* elbo;
    double* grad;
    int D, S;
    double scale, tau, c0;   // c0 = D/2 log(tau / 2 pi) + D/2 (1 + log 2 pi)
    bsc_adam adam;
};

__global__ __launch_bounds__(FIN_BLOCK) void glm_update_kernel(GlmArgs a) {
    __shared__ double red[FIN_WAVES][BSC_WAVE];
    __shared__ double sh[2 * MAX_S + 16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, S = a.S;
    const int n_chunks = (D + 7) / 8;
    const int chunk = (int)blockIdx.x;   // == n_chunks: the scalar workgroup
    const double inv_S = 1.0 / (double)S;

    if (chunk < n_chunks) {
        // ---------------- column workgroup: columns d0 .. d0 + 7 ----------------
        const int d0 = 8 * chunk;
        const int dl = lane >> 3, sl = lane & 7;  // slab order within the run is [d][s]
        const int d = d0 + dl;
        double gm = 0.0, gr = 0.0;
        // every small operand of wave 0 is requested before the slab: one memory round trip for the workgroup
        double p_m = 0.0, p_rho = 0.0, p_m1 = 0.0, p_m2 = 0.0, p_r1 = 0.0, p_r2 = 0.0, e_next = 0.0;
        if (wave == 0) {
            if (sl == 0 && d < D) {
                p_m = a.lam_in[d]; p_rho = a.lam_in[D + d];
                p_m1 = a.m1[d]; p_m2 = a.m2[d];
                p_r1 = a.m1[D + d]; p_r2 = a.m2[D + d];
            }
            if (a.eps_next && sl < S && d < D) e_next = a.eps_next[(int64_t)sl * (D + 1) + d];
        }
        if (a.slab) {  // S <= 8: lane <-> (column dl, draw sl) of one 256-byte slab run
            const bool live = sl < S && d < D;
            double wv = 0.0, ev = 0.0;
            if (wave == 0 && live) {
                wv = (double)a.W[(int64_t)sl * D + d];
                ev = a.eps[(int64_t)sl * (D + 1) + d];
            }
            double s4[4];
            slab_run_sum<SLAB_STRIDE, FIN_WAVES>(a.slab, a.n_slab, 64 * chunk, wave, lane, s4, [] {});
            if (lane < 16) {
#pragma unroll
                for (int i = 0; i < 4; ++i) red[wave][4 * lane + i] = s4[i];
            }
            __syncthreads();
            if (wave != 0) return;
            double g = red[0][lane];
#pragma unroll
            for (int k = 1; k < FIN_WAVES; ++k) g += red[k][lane];
            if (live) {
                gm = a.scale * g - a.tau * wv;
                gr = gm * ev;
            }
        } else {
            if (wave != 0) return;
            for (int s = sl; s < S; s += 8) {
                if (d < D) {
                    const double wv = (double)a.W[(int64_t)s * D + d];
                    const double dw = a.scale * a.stats[S + (int64_t)s * D + d] - a.tau * wv;
                    gm += dw;
                    gr += dw * a.eps[(int64_t)s * (D + 1) + d];
                }
            }
        }
        // fold the 8 draw lanes (lane bits 0-2)
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            gm += __shfl_xor(gm, off);
            gr += __shfl_xor(gr, off);
        }
        double* new_m = sh;        // [8]
        double* new_sd = sh + 8;   // [8]
        if (sl == 0 && d < D) {
            const double g_m = gm * inv_S;
            const double g_r = gr * inv_S * exp(p_rho) + 1.0;
            a.grad[d] = g_m;
            a.grad[D + d] = g_r;
            const double nm = bsc_adam_ascent<true>(p_m, g_m, p_m1, p_m2, a.adam);
            a.m1[d] = p_m1; a.m2[d] = p_m2;
            const double nr = bsc_adam_ascent<true>(p_rho, g_r, p_r1, p_r2, a.adam);
            a.m1[D + d] = p_r1; a.m2[D + d] = p_r2;
            a.lam_out[d] = nm;
            a.lam_out[D + d] = nr;
            new_m[dl] = nm;
            new_sd[dl] = exp(nr);
        }
        wave_lds_sync();
        if (a.eps_next && d < D) {   // w = m + e^rho eps for this lane's (column, draws sl, sl + 8, ...)
            for (int s = sl; s < S; s += 8) {
                const double en = s == sl ? e_next : a.eps_next[(int64_t)s * (D + 1) + d];
                a.W_next[(int64_t)s * D + d] = (float)(new_m[dl] + new_sd[dl] * en);
            }
        }
        return;
    }

    // ---------------------------- scalar workgroup ----------------------------
    double* ells = sh;             // [S]
    double* wsq = sh + MAX_S;      // [S]
    double rho_part = 0.0;
    for (int d = tid; d < D; d += FIN_BLOCK) rho_part += a.lam_in[D + d];
    if (a.slab) {  // S <= 8: thread -> (draw tid & 7, slab-row group tid >> 3)
        double part = slab_column_sum<SLAB_STRIDE, 8>(a.slab + SLAB_G + (tid & 7), tid >> 3, FIN_BLOCK / 8, a.n_slab);
        part += __shfl_xor(part, 8);
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        if (lane < 8) red[wave][lane] = part;
    } else {
        for (int s = tid; s < S; s += FIN_BLOCK) ells[s] = a.stats[s];
    }
    // |w_s|^2: a wave per draw, fixed order
    for (int s = wave; s < S; s += FIN_WAVES) {
        double part = 0.0;
        for (int d = lane; d < D; d += BSC_WAVE) {
            const double wv = (double)a.W[(int64_t)s * D + d];
            part += wv * wv;
        }
        part = wave_allsum_f64(part);
        if (lane == 0) wsq[s] = part;
    }
    rho_part = wave_allsum_f64(rho_part);
    if (lane == 0) red[wave][32] = rho_part;  // column 32: clear of the ell staging columns
    __syncthreads();
    if (a.slab && tid < 8) {
        double t = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) t += red[k][tid];
        ells[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double sum_rho = 0.0;
        for (int k = 0; k < FIN_WAVES; ++k) sum_rho += red[k][32];
        double fsum = 0.0;
        for (int s = 0; s < S; ++s) fsum += a.scale * ells[s] - 0.5 * a.tau * wsq[s];
        a.elbo[0] = fsum * inv_S + a.c0 + sum_rho;
    }
}

// ---- host side (pass_rows and check_glm_obs_args: csrc/bsc_glm_pass.h, shared with csrc/bsc_glm_group.hip) ---------

// the link, then the envelope of every regression pass
int check_glm_args(const char* who, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                   const float* W, int32_t S, int max_s) {
    BSC_REQUIRE(link == BSC_GLM_LOGISTIC || link == BSC_GLM_POISSON,
                "%s: link=%d must be BSC_GLM_LOGISTIC (0) or BSC_GLM_POISSON (1)", who, link);
    BSC_REQUIRE(y || B <= 0, "%s: null pointer", who);
    return check_regress_args(who, X, ldx, B, D, W, S, max_s);
}

template <int LINK>
void launch_pass_link(bsc_ctx* ctx, const float* X, int64_t ldx, const float* y, int64_t B, int D, const float* W,
                      int sg, PassGrid g, float* slab) {
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, B, tail...);
    };
    launch_pass_shape(pass_rows(D, y), D, [&] { go(glm_pass_mfma_kernel<LINK>, W, sg, slab, g.n_iter); },
                      [&](auto full) { go(glm_pass_kernel<LINK, decltype(full)::value>, D, W, sg, slab, g.n_iter); });
}

// o, v: the offset and the weight; with neither, the kernels of this file
void launch_pass(bsc_ctx* ctx, int link, const float* X, int64_t ldx, const float* y, const float* o, const float* v,
                 int64_t B, int D, const float* W, int sg, PassGrid g, float* slab) {
    if (o || v)
        bsc_glm_obs_launch_pass(ctx, link, pass_rows(D, y, o, v) == MT_ROWS, X, ldx, y, o, v, B, D, W, sg, g.n_blocks,
                                g.n_iter, slab);
    else if (link == BSC_GLM_LOGISTIC) launch_pass_link<BSC_GLM_LOGISTIC>(ctx, X, ldx, y, B, D, W, sg, g, slab);
    else launch_pass_link<BSC_GLM_POISSON>(ctx, X, ldx, y, B, D, W, sg, g, slab);
}

int slab_for(bsc_ctx* ctx, PassGrid g, float** slab) {
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, (size_t)g.n_blocks * SLAB_STRIDE * sizeof(float), &ws);
    *slab = (float*)ws;
    return rc;
}

// The pass for S <= 8 draws, its block partials left in the workspace for the finish.
int pass_partial_impl(bsc_ctx* ctx, int link, const float* X, int64_t ldx, const float* y, const float* o,
                      const float* v, int64_t B, int32_t D, const float* W, int32_t S) {
    const PassGrid g = pass_grid(ctx, B, pass_rows(D, y, o, v));
    float* slab = nullptr;
    const int rc = slab_for(ctx, g, &slab);
    if (rc != BSC_OK) return rc;
    {
        bsc_prof_scope prof(ctx);  // times the pass kernel alone
        launch_pass(ctx, link, X, ldx, y, o, v, B, (int)D, W, (int)S, g, slab);
    }
    BSC_LAUNCH_CHECK();
    ctx->slab_rows = g.n_blocks;
    return BSC_OK;
}

// The pass over all S draws, eight per launch, each reduced into ell and G in float64.
int data_pass_impl(bsc_ctx* ctx, const char* who, int link, const float* X, int64_t ldx, const float* y, const float* o,
                   const float* v, int64_t B, int32_t D, const float* W, int32_t S, double* ell, double* G) {
    BSC_REQUIRE(ell && G, "%s: null output", who);
    const PassGrid g = pass_grid(ctx, B, pass_rows(D, y, o, v));
    float* slab = nullptr;
    const int rc = slab_for(ctx, g, &slab);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    const dim3 rgrid((SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) { launch_pass(ctx, link, X, ldx, y, o, v, B, (int)D, W + (int64_t)s0 * D, sg, g, slab); },
        [&](int s0) {
            hipLaunchKernelGGL(glm_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, slab, g.n_blocks, (int)D,
                               (int)S, s0, ell, G);
        });
}

int update_impl(bsc_ctx* ctx, const char* who, const double* stats, const double* lam_in, double* lam_out, double* m1,
                double* m2, const double* eps, const float* W, int32_t D, int32_t S, double scale, double tau, int64_t t,
                double lr, double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                double* eps_next, int32_t eps_next_ready, float* W_next, double* elbo, double* grad) {
    int rc = check_meanfield_update(who, lam_in && lam_out && m1 && m2 && eps && W && elbo && grad, lam_in, lam_out, D, S,
                                    MAX_S, tau, /*has_gamma=*/false, 0.0, 0.0, scale, t);
    if (rc != BSC_OK) return rc;
    GlmArgs a;
    a.stats = stats;
    a.slab = nullptr;
    a.n_slab = 0;
    if (!stats) {
        BSC_REQUIRE(ctx->slab_rows > 0 && ctx->workspace, "%s: stats is null and no pass partials are pending", who);
        BSC_REQUIRE(S <= SG && D <= GCOLS, "%s: slab input needs S<=8, D<=256", who);
        a.slab = (const float*)ctx->workspace;
        a.n_slab = ctx->slab_rows;
    }
    // (the noise of next_step is drawn here off the default path only: drivers draw ahead)
    rc = next_draw_noise(ctx, who, /*has_extra=*/false, eps, W, nullptr, eps_next, W_next, nullptr, D, S, seed, next_step,
                         eps_next_ready);
    if (rc != BSC_OK) return rc;
    a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.eps_next = eps_next; a.W_next = W_next;
    a.elbo = elbo; a.grad = grad;
    a.D = D; a.S = S;
    a.scale = scale; a.tau = tau;
    a.c0 = 0.5 * (double)D * (log(tau) - BSC_LOG_2PI) + 0.5 * (double)D * (1.0 + BSC_LOG_2PI);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish kernel, timed apart from the pass
        hipLaunchKernelGGL(glm_update_kernel, dim3((D + 7) / 8 + 1), dim3(FIN_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    if (!stats) ctx->slab_rows = 0;   // the partials are consumed
    return BSC_OK;
}

}  // namespace

extern "C" {

int bsc_glm_data_pass(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                      const float* W, int32_t S, double* ell, double* G) {
    BSC_CHECK_CTX(ctx);
    const int rc = check_glm_args("bsc_glm_data_pass", link, X, ldx, y, B, D, W, S, MAX_S);
    if (rc != BSC_OK) return rc;
    return data_pass_impl(ctx, "bsc_glm_data_pass", link, X, ldx, y, nullptr, nullptr, B, D, W, S, ell, G);
}

int bsc_glm_data_pass_obs(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, const float* offset,
                          const float* weight, int64_t B, int32_t D, const float* W, int32_t S, double* ell,
                          double* G) {
    BSC_CHECK_CTX(ctx);
    const int rc = check_glm_obs_args("bsc_glm_data_pass_obs", link, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc != BSC_OK) return rc;
    return data_pass_impl(ctx, "bsc_glm_data_pass_obs", link, X, ldx, y, offset, weight, B, D, W, S, ell, G);
}

int bsc_glm_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1, double* m2,
                   const double* eps, const float* W, int32_t D, int32_t S, double scale, double prior_precision,
                   int64_t t, double lr, double beta1, double beta2, double adam_eps, uint64_t seed, uint32_t next_step,
                   double* eps_next, int32_t eps_next_ready, float* W_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    return update_impl(ctx, "bsc_glm_update", stats, lam_in, lam_out, m1, m2, eps, W, D, S, scale, prior_precision, t, lr,
                       beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, elbo, grad);
}

int bsc_glm_pass_update(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y, int64_t B, int32_t D,
                        const double* lam_in, double* lam_out, double* m1, double* m2, const double* eps, const float* W,
                        int32_t S, double scale, double prior_precision, int64_t t, double lr, double beta1, double beta2,
                        double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                        float* W_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    int rc = check_glm_args("bsc_glm_pass_update", link, X, ldx, y, B, D, W, S, SG);
    if (rc != BSC_OK) return rc;
    rc = pass_partial_impl(ctx, link, X, ldx, y, nullptr, nullptr, B, D, W, S);
    if (rc != BSC_OK) return rc;
    return update_impl(ctx, "bsc_glm_pass_update", nullptr, lam_in, lam_out, m1, m2, eps, W, D, S, scale, prior_precision,
                       t, lr, beta1, beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, elbo, grad);
}

int bsc_glm_pass_update_obs(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y,
                            const float* offset, const float* weight, int64_t B, int32_t D, const double* lam_in,
                            double* lam_out, double* m1, double* m2, const double* eps, const float* W, int32_t S,
                            double scale, double prior_precision, int64_t t, double lr, double beta1, double beta2,
                            double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next, int32_t eps_next_ready,
                            float* W_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_pass_update_obs";
    int rc = check_glm_obs_args(who, link, X, ldx, y, offset, weight, B, D, W, S, SG);
    if (rc != BSC_OK) return rc;
    rc = pass_partial_impl(ctx, link, X, ldx, y, offset, weight, B, D, W, S);
    if (rc != BSC_OK) return rc;
    return update_impl(ctx, who, nullptr, lam_in, lam_out, m1, m2, eps, W, D, S, scale, prior_precision, t, lr, beta1,
                       beta2, adam_eps, seed, next_step, eps_next, eps_next_ready, W_next, elbo, grad);
}

}  // extern "C"
