// Random-intercept logistic / Poisson regression on the fused pathwise pass: csrc/bsc_glm_pass.h's OBS bodies with the
// group flag on, the per-group sums of the residuals, and the finish for the latent z = [w (D) | b (J) | zeta].
//
//     l[n,s] = x_n . w_s + b_s[g_n] + o_n
//     ell[s] = sum_n v_n (y_n l_ns - A(l_ns))      G[s,:] = sum_n r_ns x_n      H[s,j] = sum_{n : g_n = j} r_ns
// with r_ns = v_n (y_n - A'(l_ns)).  ell and G leave through the slab as in csrc/bsc_glm.hip.  H is a scatter; it is
// done without float atomics, in an order that depends on the group plan alone:
//
//   plan     bsc_glm_group_plan (host, plain C++, once per batch): the rows in stable order by group, each group's run
//            cut into segments of at most BSC_GLM_GROUP_SEG_ROWS rows, a (start, length, group) table and every
//            group's first segment.  The only place ids are range-checked, which is why it synchronises.
//   pass     the six kernels below; besides the slab they leave every residual in R, 32 bytes per row in 16-row blocks
//            [block][draw][row] (the MFMA tile's live lanes store 16 bytes each).
//   segment  glm_group_segment_kernel: one wave per plan segment, 8 row-lanes x 8 draws; a row-lane strides the
//            segment's rows through the plan's permutation, accumulates in float64, and the eight row-lanes fold by a
//            fixed shuffle tree.
//   group    glm_group_sum_kernel: a group's segments added in segment order, in float64, into H[S][J]; a group
//            without rows gets exactly 0.
//
// The finish (bsc_glm_hier_update) is two launches: the per-draw scalars in fixed order, then one thread per
// coordinate of lam for the gradient, Adam and the next draws.  Both bodies are csrc/bsc_meanfield.h's, shared with
// csrc/bsc_glm_nb.hip; HierModel below is what this model adds to them.
#include <vector>

#include "bsc_group_sum.h"
#include "bsc_meanfield.h"

namespace {

constexpr int MAX_S = 64;

// (The plan layout and the two kernels of the group sums: csrc/bsc_group_sum.h, shared with
// csrc/bsc_glm_scalar_group.hip.)

// ---- the six pass kernels -------------------------------------------------------------------------------------------

template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_group_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, int S, float* __restrict__ slab,
    int n_iter, GlmGroupArgs ga) {
    glm_pass_body<GlmFamily<LINK>, FULL, true, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, &ga);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_group_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, int S, float* __restrict__ slab, int n_iter,
    GlmGroupArgs ga) {
    glm_pass_mfma_body<GlmFamily<LINK>, true, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, &ga);
}

__global__ __launch_bounds__(RED_BLOCK) void glm_group_slab_reduce_kernel(const float* __restrict__ slab, int n_blocks,
                                                                          int D, int S, int s_base,
                                                                          double* __restrict__ ell,
                                                                          double* __restrict__ G) {
    regress_slab_reduce(slab, n_blocks, D, S, s_base, ell, G);
}

// ---- the finish -----------------------------------------------------------------------------------------------------

// z = [w (D) | b (J) | zeta]; scal = [ez (64) | g_zeta (64) | f (64) | sum rho];
// c0 = D/2 log(prec / 2 pi) - J/2 log 2 pi + a0 log b0 - lnGamma(a0).
struct HierModel : MeanfieldArgs {
    const float* Bz;         // [ceil(S / 8)][J][8]
    float* Bz_next;
    int J;

    static constexpr int N_SLOTS = 3;
    static constexpr bool LAST_HAS_NEXT = false;   // zeta's next draw is made where it is used, in float64

    // sum_j b_sj^2
    static __device__ __forceinline__ double extra_sq(const HierModel& a, int s, double* red) {
        const int J = a.J;
        double pb = 0.0;
        const float* bz = a.Bz + (int64_t)(s >> 3) * J * SG + (s & 7);
        for (int j = threadIdx.x; j < J; j += MF_BLOCK) {
            const double bv = (double)bz[(int64_t)j * SG];
            pb += bv * bv;
        }
        return block_sum_f64<MF_WAVES>(pb, red);
    }

    // zeta_s, g_zeta and f_s = scale ell_s + log p(z_s)
    static __device__ __forceinline__ void draw_scalars(const HierModel& a, int s, double wsq, double bsq) {
        const int J = a.J, P = a.P;
        const double zeta = a.lam_in[P - 1] + exp(a.lam_in[2 * P - 1]) * a.eps[(int64_t)s * P + P - 1];
        const double ez = exp(zeta);
        a.scal[s] = ez;
        a.scal[MF_MAX_S + s] = 0.5 * (double)J + a.a0 - ez * (a.b0 + 0.5 * bsq);
        a.scal[2 * MF_MAX_S + s] = a.scale * a.stats[s] + a.c0 - 0.5 * a.prec * wsq + 0.5 * (double)J * zeta -
                                   0.5 * ez * bsq + a.a0 * zeta - a.b0 * ez;
    }

    // b_j from H (behind G in stats) and the draw's precision e^zeta; zeta from g_zeta
    static __device__ __forceinline__ double grad_term(const HierModel& a, int i, int s) {
        const int D = a.D, J = a.J, S = a.S;
        if (i == a.P - 1) return a.scal[MF_MAX_S + s];
        const double* H = a.stats + S + (int64_t)S * D;
        const int j = i - D;
        const double bv = (double)a.Bz[((int64_t)(s >> 3) * J + j) * SG + (s & 7)];
        return a.scale * H[(int64_t)s * J + j] - a.scal[s] * bv;
    }

    static __device__ __forceinline__ void store_next(const HierModel& a, int i, double nm, double sd) {
        const int J = a.J, S = a.S, P = a.P;
        const int j = i - a.D;
        const int s_pad = (S + SG - 1) / SG * SG;      // the unused slots of the last chunk stay zero
        for (int s = 0; s < s_pad; ++s)
            a.Bz_next[((int64_t)(s >> 3) * J + j) * SG + (s & 7)] =
                s < S ? (float)(nm + sd * a.eps_next[(int64_t)s * P + i]) : 0.f;
    }
};

__global__ __launch_bounds__(MF_BLOCK) void glm_hier_scalars_kernel(HierModel a) { meanfield_scalars_body(a); }

__global__ __launch_bounds__(MF_BLOCK) void glm_hier_coord_kernel(HierModel a) { meanfield_coord_body(a); }

// ---- host side ------------------------------------------------------------------------------------------------------

template <int LINK>
void launch_group_link(bsc_ctx* ctx, int rows, const float* X, int64_t ldx, const float* y, const float* o,
                       const float* v, int64_t B, int D, const float* W, int sg, PassGrid g, float* slab,
                       const GlmGroupArgs& ga) {
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, o, v, B, tail...);
    };
    launch_pass_shape(
        rows, D, [&] { go(glm_group_pass_mfma_kernel<LINK>, W, sg, slab, g.n_iter, ga); },
        [&](auto full) { go(glm_group_pass_kernel<LINK, decltype(full)::value>, D, W, sg, slab, g.n_iter, ga); });
}

}  // namespace

extern "C" {

int64_t bsc_glm_group_plan_size(int64_t B, int32_t J) {
    if (B < 0 || B > BSC_GLM_GROUP_MAX_ROWS || J < 1 || J > BSC_GLM_GROUP_MAX_J) return -1;
    return plan_seg_off(B, J) + 3 * plan_seg_bound(B, J);
}

int bsc_glm_group_plan_host(const int32_t* g, int64_t B, int32_t J, int32_t* plan, int32_t* n_segments) {
    const char* who = "bsc_glm_group_plan_host";
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE(B >= 0 && B <= BSC_GLM_GROUP_MAX_ROWS, "%s: B=%lld must be in [0,%lld]", who, (long long)B,
                (long long)BSC_GLM_GROUP_MAX_ROWS);
    BSC_REQUIRE(plan && (g || B == 0), "%s: null pointer", who);
    // counting sort: counts, then every row to the next free slot of its group, rows ascending
    std::vector<int64_t> next((size_t)J + 1, 0);
    for (int64_t n = 0; n < B; ++n) {
        BSC_REQUIRE(g[n] >= 0 && g[n] < J, "%s: row %lld has group id %d outside [0,%d)", who, (long long)n, g[n], J);
        ++next[(size_t)g[n] + 1];
    }
    for (int j = 0; j < J; ++j) next[j + 1] += next[j];   // next[j]: where group j starts
    int32_t* perm = plan + plan_perm_off();
    int32_t* grp = plan + plan_grp_off(B);
    int32_t* tab = plan + plan_seg_off(B, J);
    int64_t n_seg = 0;
    for (int j = 0; j < J; ++j) {
        grp[j] = (int32_t)n_seg;
        for (int64_t at = next[j]; at < next[j + 1]; at += SEG_ROWS) {
            const int64_t len = next[j + 1] - at < SEG_ROWS ? next[j + 1] - at : SEG_ROWS;
            tab[3 * n_seg] = (int32_t)at;
            tab[3 * n_seg + 1] = (int32_t)len;
            tab[3 * n_seg + 2] = j;
            ++n_seg;
        }
    }
    grp[J] = (int32_t)n_seg;
    for (int64_t n = 0; n < B; ++n) perm[next[g[n]]++] = (int32_t)n;
    plan[0] = PLAN_MAGIC;
    plan[1] = (int32_t)B;
    plan[2] = J;
    plan[3] = (int32_t)n_seg;
    plan[4] = SEG_ROWS;
    plan[5] = plan[6] = plan[7] = 0;
    if (n_segments) *n_segments = (int32_t)n_seg;
    return BSC_OK;
}

int bsc_glm_group_plan(bsc_ctx* ctx, const int32_t* g, int64_t B, int32_t J, int32_t* plan, int32_t* n_segments) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_group_plan";
    BSC_REQUIRE(!ctx->capturing, "%s inside a graph capture", who);
    const int64_t n = bsc_glm_group_plan_size(B, J);
    BSC_REQUIRE(n >= 0, "%s: B=%lld J=%d (B in [0,%lld], J in [1,%d])", who, (long long)B, J,
                (long long)BSC_GLM_GROUP_MAX_ROWS, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE(plan && (g || B == 0), "%s: null pointer", who);
    std::vector<int32_t> hg((size_t)B), hp((size_t)n, 0);
    BSC_HIP(hipStreamSynchronize(ctx->stream));      // g may have been written on the stream
    if (B) BSC_HIP(hipMemcpy(hg.data(), g, (size_t)B * 4, hipMemcpyDeviceToHost));
    int32_t n_seg = 0;
    const int rc = bsc_glm_group_plan_host(hg.data(), B, J, hp.data(), &n_seg);
    if (rc != BSC_OK) return rc;
    BSC_HIP(hipMemcpy(plan, hp.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    if (n_segments) *n_segments = n_seg;
    return BSC_OK;
}

int64_t bsc_glm_group_workspace_bytes(bsc_ctx* ctx, int64_t B, int32_t J) {
    if (!ctx || B < 0 || J < 1) return -1;
    const PassGrid g8 = pass_grid(ctx, B, ROWS), g16 = pass_grid(ctx, B, MT_ROWS);
    const int nb = g8.n_blocks > g16.n_blocks ? g8.n_blocks : g16.n_blocks;
    return (int64_t)(round256((size_t)nb * SLAB_STRIDE * 4) + round256((size_t)((B + 15) / 16) * R_BLOCK * 4) +
                     (size_t)(plan_seg_bound(B, J) + 1) * SG * 8);
}

int bsc_glm_data_pass_groups(bsc_ctx* ctx, int32_t link, const float* X, int64_t ldx, const float* y,
                             const float* offset, const float* weight, const int32_t* g, const int32_t* plan, int64_t B,
                             int32_t D, int32_t J, const float* W, const float* Bz, int32_t S, double* ell, double* G,
                             double* H) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_data_pass_groups";
    const int rc0 = check_glm_obs_args(who, link, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc0 != BSC_OK) return rc0;
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE(B <= BSC_GLM_GROUP_MAX_ROWS, "%s: B=%lld is more than a group plan holds (%lld)", who, (long long)B,
                (long long)BSC_GLM_GROUP_MAX_ROWS);
    BSC_REQUIRE(g || B == 0, "%s: g is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)g) & 3) == 0, "%s: g must be 4-byte aligned", who);
    BSC_REQUIRE(plan, "%s: plan is null (bsc_glm_group_plan builds it)", who);
    BSC_REQUIRE(Bz && (((uintptr_t)Bz) & 3) == 0, "%s: Bz is null or not 4-byte aligned", who);
    BSC_REQUIRE(ell && G, "%s: null output", who);
    BSC_REQUIRE(H, "%s: H is null", who);

    const int rows = pass_rows(D, y, offset, weight, g);
    const PassGrid pg = pass_grid(ctx, B, rows);
    const int64_t r_blocks = (B + 15) / 16;
    const int64_t seg_bound = plan_seg_bound(B, J);
    const size_t slab_bytes = round256((size_t)pg.n_blocks * SLAB_STRIDE * 4);
    const size_t r_bytes = round256((size_t)r_blocks * R_BLOCK * 4);
    void* ws = nullptr;
    const int rc = bsc_workspace(ctx, slab_bytes + r_bytes + (size_t)(seg_bound + 1) * SG * 8, &ws);
    if (rc != BSC_OK) return rc;
    ctx->slab_rows = 0;  // the slab is consumed here
    float* slab = (float*)ws;
    GlmGroupArgs ga;
    ga.g = g;
    ga.J = J;
    ga.R = (float*)((char*)ws + slab_bytes);
    ga.r_blocks = r_blocks;
    double* segsum = (double*)((char*)ws + slab_bytes + r_bytes);

    const dim3 rgrid((SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {
            ga.Bz = Bz + (int64_t)(s0 / SG) * J * SG;
            if (link == BSC_GLM_LOGISTIC)
                launch_group_link<BSC_GLM_LOGISTIC>(ctx, rows, X, ldx, y, offset, weight, B, D, W + (int64_t)s0 * D, sg,
                                                    pg, slab, ga);
            else
                launch_group_link<BSC_GLM_POISSON>(ctx, rows, X, ldx, y, offset, weight, B, D, W + (int64_t)s0 * D, sg,
                                                   pg, slab, ga);
        },
        [&](int s0) {
            hipLaunchKernelGGL(glm_group_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream, slab, pg.n_blocks,
                               (int)D, (int)S, s0, ell, G);
        },
        [&](int s0) -> int {   // the chunk's group sums
            return launch_group_sums(ctx, plan, B, (int)J, seg_bound, (const float*)ga.R, segsum, (int)S, s0, H);
        });
}

int bsc_glm_hier_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                        double* m2, const double* eps, const float* W, const float* Bz, int32_t D, int32_t J, int32_t S,
                        double scale, double prior_precision, double a0, double b0, int64_t t, double lr, double beta1,
                        double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                        int32_t eps_next_ready, float* W_next, float* Bz_next, double* elbo, double* grad) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_hier_update";
    BSC_REQUIRE(stats, "%s: stats is null (pending pass partials are not read: pass [ell | G | H])", who);
    int rc = check_meanfield_update(who, lam_in && lam_out && m1 && m2 && eps && W && Bz && elbo && grad, lam_in, lam_out,
                                    D, S, MAX_S, prior_precision, /*has_gamma=*/true, a0, b0, scale, t);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    const int P = D + J + 1;
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, Bz, eps_next, W_next, Bz_next, P - 1, S, seed, next_step,
                         eps_next_ready);
    if (rc != BSC_OK) return rc;
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (HierModel::N_SLOTS * MAX_S + 8) * sizeof(double), &ws);
    if (rc != BSC_OK) return rc;
    HierModel a;
    a.stats = stats; a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.Bz = Bz; a.eps_next = eps_next; a.W_next = W_next; a.Bz_next = Bz_next;
    a.scal = (double*)ws; a.elbo = elbo; a.grad = grad;
    a.D = D; a.J = J; a.S = S; a.P = P;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) - 0.5 * (double)J * BSC_LOG_2PI + a0 * log(b0) -
           lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    ctx->slab_rows = 0;   // the workspace is this finish's now
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish, timed apart from the pass
        hipLaunchKernelGGL(glm_hier_scalars_kernel, dim3(S + 1), dim3(MF_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(glm_hier_coord_kernel, dim3((P + MF_BLOCK - 1) / MF_BLOCK), dim3(MF_BLOCK), 0, ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
