// Random intercepts for the regression families with a learned scalar -- the negative binomial's dispersion, the Gamma
// shape, the Weibull shape with right censoring -- on the fused pathwise pass: csrc/bsc_glm_pass.h's bodies with the
// group flag on and a scalar family (csrc/bsc_families.h; with_scalar_family maps the public id to it), the per-group
// sums of the residuals (csrc/bsc_group_sum.h), and the finish for the latent z = [w (D) | b (J) | zeta | tau].
//
//     l[n,s] = x_n . w_s + b_s[g_n] + o_n            y_n ~ F(l_ns, e^{tau_s})        (the families' links, unchanged)
//     ell[s], G[s,:] = sum_n r_ns x_n, T[s] = d ell[s] / d tau_s       as csrc/bsc_scalar_family.h's passes leave them
//     H[s,j] = sum_{n : g_n = j} r_ns                                  as csrc/bsc_glm_group.hip's pass leaves it
// The intercept enters through l alone, so a link sees nothing new: the GRP branches of the bodies hand it the draw's
// GlmDisp and the T accumulator, the slab is NB_SLAB_STRIDE floats per workgroup and T folds as it does without groups.
// The gather sits ahead of the prefetch, the selects sit on the link's inputs, there are no float atomics, and every
// order of summation is fixed by the plan -- all of it the parents'.
//
// The finish (bsc_glm_scalar_hier_update) serves the three families: it sees stats = [ell | G | H | T], never the
// likelihood.  Two launches, csrc/bsc_meanfield.h's bodies with HierScalarModel below.
//
// A translation unit of its own so that csrc/bsc_glm_group.hip and the three family units keep their kernels, their
// names and their code.
#include "bsc_group_sum.h"
#include "bsc_meanfield.h"

namespace {

constexpr int MAX_S = 64;
static_assert(MAX_S == MF_MAX_S, "the pass and the finish take the same number of draws");

// ---- the nine pass kernels ------------------------------------------------------------------------------------------

template <int LINK, bool FULL>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_scalar_group_pass_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, int D, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter, GlmGroupArgs ga) {
    glm_pass_body<GlmFamily<LINK>, FULL, true, true>(X, ldx, y, o, v, B, D, W, S, slab, n_iter, &ga, logtau);
}

template <int LINK>
__global__ __launch_bounds__(PASS_BLOCK, 2) void glm_scalar_group_pass_mfma_kernel(
    const float* __restrict__ X, int64_t ldx, const float* __restrict__ y, const float* __restrict__ o,
    const float* __restrict__ v, int64_t B, const float* __restrict__ W, const float* __restrict__ logtau, int S,
    float* __restrict__ slab, int n_iter, GlmGroupArgs ga) {
    glm_pass_mfma_body<GlmFamily<LINK>, true, true>(X, ldx, y, o, v, B, W, S, slab, n_iter, &ga, logtau);
}

__global__ __launch_bounds__(RED_BLOCK) void glm_scalar_group_slab_reduce_kernel(
    const float* __restrict__ slab, int n_blocks, int D, int S, int s_base, double* __restrict__ ell,
    double* __restrict__ G, double* __restrict__ T) {
    regress_slab_reduce<NB_SLAB_STRIDE>(slab, n_blocks, D, S, s_base, ell, G, T);
}

// ---- the finish -----------------------------------------------------------------------------------------------------

// z = [w (D) | b (J) | zeta | tau]; scal = [ez (64) | g_zeta (64) | g_tau (64) | f (64) | sum rho];
// c0 = D/2 log(prec / 2 pi) - J/2 log 2 pi + ga0 log gb0 - lnGamma(ga0) + a0 log b0 - lnGamma(a0).
// (a0, b0) of MeanfieldArgs is tau's prior, (ga0, gb0) zeta's.
struct HierScalarModel : MeanfieldArgs {
    const float* Bz;         // [ceil(S / 8)][J][8]
    float* Bz_next;
    const float* logtau;     // [S]
    float* logtau_next;
    double ga0, gb0;
    int J;

    static constexpr int N_SLOTS = 4;
    static constexpr bool LAST_HAS_NEXT = true;    // tau's; zeta's next draw is made where it is used, in float64

    // sum_j b_sj^2
    static __device__ __forceinline__ double extra_sq(const HierScalarModel& a, int s, double* red) {
        const int J = a.J;
        double pb = 0.0;
        const float* bz = a.Bz + (int64_t)(s >> 3) * J * SG + (s & 7);
        for (int j = threadIdx.x; j < J; j += MF_BLOCK) {
            const double bv = (double)bz[(int64_t)j * SG];
            pb += bv * bv;
        }
        return block_sum_f64<MF_WAVES>(pb, red);
    }

    // zeta_s, g_zeta, g_tau and f_s = scale ell_s + log p(z_s), with tau_s the float32 value the pass read
    static __device__ __forceinline__ void draw_scalars(const HierScalarModel& a, int s, double wsq, double bsq) {
        const int D = a.D, J = a.J, S = a.S, P = a.P;
        const double zeta = a.lam_in[P - 2] + exp(a.lam_in[2 * P - 2]) * a.eps[(int64_t)s * P + P - 2];
        const double ez = exp(zeta);
        const double tau = (double)a.logtau[s];
        const double et = exp(tau);
        const double T = a.stats[S + (int64_t)S * D + (int64_t)S * J + s];
        a.scal[s] = ez;
        a.scal[MF_MAX_S + s] = 0.5 * (double)J + a.ga0 - ez * (a.gb0 + 0.5 * bsq);
        a.scal[2 * MF_MAX_S + s] = a.scale * T + a.a0 - a.b0 * et;
        a.scal[3 * MF_MAX_S + s] = a.scale * a.stats[s] + a.c0 - 0.5 * a.prec * wsq + 0.5 * (double)J * zeta -
                                   0.5 * ez * bsq + a.ga0 * zeta - a.gb0 * ez + a.a0 * tau - a.b0 * et;
    }

    // b_j from H (behind G in stats) and the draw's precision e^zeta; zeta and tau from their slots
    static __device__ __forceinline__ double grad_term(const HierScalarModel& a, int i, int s) {
        const int D = a.D, J = a.J, S = a.S;
        if (i == a.P - 1) return a.scal[2 * MF_MAX_S + s];
        if (i == a.P - 2) return a.scal[MF_MAX_S + s];
        const double* H = a.stats + S + (int64_t)S * D;
        const int j = i - D;
        const double bv = (double)a.Bz[((int64_t)(s >> 3) * J + j) * SG + (s & 7)];
        return a.scale * H[(int64_t)s * J + j] - a.scal[s] * bv;
    }

    static __device__ __forceinline__ void store_next(const HierScalarModel& a, int i, double nm, double sd) {
        const int J = a.J, S = a.S, P = a.P;
        if (i == P - 2) return;                        // zeta has no next-draw buffer
        if (i == P - 1) {
            for (int s = 0; s < S; ++s) a.logtau_next[s] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
            return;
        }
        const int j = i - a.D;
        const int s_pad = (S + SG - 1) / SG * SG;      // the unused slots of the last chunk stay zero
        for (int s = 0; s < s_pad; ++s)
            a.Bz_next[((int64_t)(s >> 3) * J + j) * SG + (s & 7)] =
                s < S ? (float)(nm + sd * a.eps_next[(int64_t)s * P + i]) : 0.f;
    }
};

__global__ __launch_bounds__(MF_BLOCK) void glm_scalar_hier_scalars_kernel(HierScalarModel a) {
    meanfield_scalars_body(a);
}

__global__ __launch_bounds__(MF_BLOCK) void glm_scalar_hier_coord_kernel(HierScalarModel a) { meanfield_coord_body(a); }

// ---- host side ------------------------------------------------------------------------------------------------------

template <class F>
void launch_scalar_group_link(bsc_ctx* ctx, int rows, const float* X, int64_t ldx, const float* y, const float* o,
                              const float* v, int64_t B, int D, const float* W, const float* logtau, int sg, PassGrid g,
                              float* slab, const GlmGroupArgs& ga) {
    constexpr int LINK = F::GLM_ID;
    const auto go = [&](auto kernel, auto... tail) {
        hipLaunchKernelGGL(kernel, dim3(g.n_blocks), dim3(PASS_BLOCK), 0, ctx->stream, X, ldx, y, o, v, B, tail...);
    };
    launch_pass_shape(
        rows, D, [&] { go(glm_scalar_group_pass_mfma_kernel<LINK>, W, logtau, sg, slab, g.n_iter, ga); },
        [&](auto full) {
            go(glm_scalar_group_pass_kernel<LINK, decltype(full)::value>, D, W, logtau, sg, slab, g.n_iter, ga);
        });
}

}  // namespace

extern "C" {

int64_t bsc_glm_scalar_group_workspace_bytes(bsc_ctx* ctx, int64_t B, int32_t J) {
    if (!ctx || B < 0 || J < 1) return -1;
    const PassGrid g8 = pass_grid(ctx, B, ROWS), g16 = pass_grid(ctx, B, MT_ROWS);
    const int nb = g8.n_blocks > g16.n_blocks ? g8.n_blocks : g16.n_blocks;
    return (int64_t)(round256((size_t)nb * NB_SLAB_STRIDE * 4) + round256((size_t)((B + 15) / 16) * R_BLOCK * 4) +
                     (size_t)(plan_seg_bound(B, J) + 1) * SG * 8);
}

int bsc_glm_scalar_data_pass_groups(bsc_ctx* ctx, int32_t family, const float* X, int64_t ldx, const float* y,
                                    const float* offset, const float* weight, const int32_t* g, const int32_t* plan,
                                    int64_t B, int32_t D, int32_t J, const float* W, const float* Bz,
                                    const float* logtau, int32_t S, double* ell, double* G, double* H, double* T) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_scalar_data_pass_groups";
    BSC_REQUIRE(scalar_family_ok(family),
                "%s: family=%d must be BSC_SCALAR_NEGBIN (0), BSC_SCALAR_GAMMA (1) or BSC_SCALAR_WEIBULL (2)", who,
                family);
    const int rc0 = check_glm_obs_args(who, BSC_GLM_LOGISTIC, X, ldx, y, offset, weight, B, D, W, S, MAX_S);
    if (rc0 != BSC_OK) return rc0;
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE(B <= BSC_GLM_GROUP_MAX_ROWS, "%s: B=%lld is more than a group plan holds (%lld)", who, (long long)B,
                (long long)BSC_GLM_GROUP_MAX_ROWS);
    BSC_REQUIRE(g || B == 0, "%s: g is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)g) & 3) == 0, "%s: g must be 4-byte aligned", who);
    BSC_REQUIRE(plan, "%s: plan is null (bsc_glm_group_plan builds it)", who);
    BSC_REQUIRE(Bz && (((uintptr_t)Bz) & 3) == 0, "%s: Bz is null or not 4-byte aligned", who);
    BSC_REQUIRE(logtau, "%s: logtau is null", who);
    BSC_REQUIRE((((uintptr_t)logtau) & 3) == 0, "%s: logtau must be 4-byte aligned", who);
    BSC_REQUIRE(ell && G && T, "%s: null output", who);
    BSC_REQUIRE(H, "%s: H is null", who);

    const int rows = pass_rows(D, y, offset, weight, g);
    const PassGrid pg = pass_grid(ctx, B, rows);
    const int64_t r_blocks = (B + 15) / 16;
    const int64_t seg_bound = plan_seg_bound(B, J);
    const size_t slab_bytes = round256((size_t)pg.n_blocks * NB_SLAB_STRIDE * 4);
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

    const dim3 rgrid((NB_SLAB_STRIDE + BSC_WAVE - 1) / BSC_WAVE);
    return for_draw_chunks(
        ctx, S,
        [&](int s0, int sg) {   // each launch with its chunk of the intercepts and of the scalar
            ga.Bz = Bz + (int64_t)(s0 / SG) * J * SG;
            const float *Ws = W + (int64_t)s0 * D, *lp = logtau + s0;
            with_scalar_family(family, [&](auto f) {
                launch_scalar_group_link<decltype(f)>(ctx, rows, X, ldx, y, offset, weight, B, D, Ws, lp, sg, pg, slab,
                                                      ga);
            });
        },
        [&](int s0) {
            hipLaunchKernelGGL(glm_scalar_group_slab_reduce_kernel, rgrid, dim3(RED_BLOCK), 0, ctx->stream,
                               (const float*)slab, pg.n_blocks, (int)D, (int)S, s0, ell, G, T);
        },
        [&](int s0) -> int {   // the chunk's group sums
            return launch_group_sums(ctx, plan, B, (int)J, seg_bound, (const float*)ga.R, segsum, (int)S, s0, H);
        });
}

int bsc_glm_scalar_hier_update(bsc_ctx* ctx, const double* stats, const double* lam_in, double* lam_out, double* m1,
                               double* m2, const double* eps, const float* W, const float* Bz, const float* logtau,
                               int32_t D, int32_t J, int32_t S, double scale, double prior_precision, double a0,
                               double b0, double group_a0, double group_b0, int64_t t, double lr, double beta1,
                               double beta2, double adam_eps, uint64_t seed, uint32_t next_step, double* eps_next,
                               int32_t eps_next_ready, float* W_next, float* Bz_next, float* logtau_next, double* elbo,
                               double* grad) {
    BSC_CHECK_CTX(ctx);
    const char* who = "bsc_glm_scalar_hier_update";
    BSC_REQUIRE(stats, "%s: stats is null (pending pass partials are not read: pass [ell | G | H | T])", who);
    int rc = check_meanfield_update(who, lam_in && lam_out && m1 && m2 && eps && W && Bz && logtau && elbo && grad,
                                    lam_in, lam_out, D, S, MAX_S, prior_precision, /*has_gamma=*/true, a0, b0, scale,
                                    t);
    if (rc != BSC_OK) return rc;
    BSC_REQUIRE(group_a0 > 0.0 && group_b0 > 0.0, "%s: group_a0=%g group_b0=%g must be positive", who, group_a0,
                group_b0);
    BSC_REQUIRE(J >= 1 && J <= BSC_GLM_GROUP_MAX_J, "%s: J=%d must be in [1,%d]", who, J, BSC_GLM_GROUP_MAX_J);
    BSC_REQUIRE((logtau_next != nullptr) == (eps_next != nullptr), "%s: next-draw buffers must be all set or all null",
                who);
    BSC_REQUIRE(!logtau_next || logtau_next != logtau, "%s: next-draw buffers must not alias the current draws", who);
    const int P = D + J + 2;
    rc = next_draw_noise(ctx, who, /*has_extra=*/true, eps, W, Bz, eps_next, W_next, Bz_next, P - 1, S, seed, next_step,
                         eps_next_ready);
    if (rc != BSC_OK) return rc;
    void* ws = nullptr;
    rc = bsc_workspace(ctx, (HierScalarModel::N_SLOTS * MAX_S + 8) * sizeof(double), &ws);
    if (rc != BSC_OK) return rc;
    HierScalarModel a;
    a.stats = stats; a.lam_in = lam_in; a.lam_out = lam_out; a.m1 = m1; a.m2 = m2;
    a.eps = eps; a.W = W; a.Bz = Bz; a.logtau = logtau;
    a.eps_next = eps_next; a.W_next = W_next; a.Bz_next = Bz_next; a.logtau_next = logtau_next;
    a.scal = (double*)ws; a.elbo = elbo; a.grad = grad;
    a.D = D; a.J = J; a.S = S; a.P = P;
    a.scale = scale; a.prec = prior_precision; a.a0 = a0; a.b0 = b0; a.ga0 = group_a0; a.gb0 = group_b0;
    a.c0 = 0.5 * (double)D * (log(prior_precision) - BSC_LOG_2PI) - 0.5 * (double)J * BSC_LOG_2PI +
           group_a0 * log(group_b0) - lgamma(group_a0) + a0 * log(b0) - lgamma(a0);
    a.adam = bsc_adam_make(lr, beta1, beta2, adam_eps, t);
    ctx->slab_rows = 0;   // the workspace is this finish's now
    {
        bsc_prof_scope prof(ctx, /*slot=*/2);  // the finish, timed apart from the pass
        hipLaunchKernelGGL(glm_scalar_hier_scalars_kernel, dim3(S + 1), dim3(MF_BLOCK), 0, ctx->stream, a);
        hipLaunchKernelGGL(glm_scalar_hier_coord_kernel, dim3((P + MF_BLOCK - 1) / MF_BLOCK), dim3(MF_BLOCK), 0,
                           ctx->stream, a);
    }
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

}  // extern "C"
