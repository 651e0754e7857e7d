// Mixture of Gaussians (BASELINE config 3): the exact posterior predictive of the fitted mixture under the
// mean-field q -- per-row log density, predictive membership and label in ONE pass over X.
//
// ABSENT in the reference: the spec is README.md:43,72 (marginalise the discrete latent by summation) applied to a NEW
// row, with the Dirichlet and the Normal-Gamma factors of svi/mog.py integrated out in closed form (a Student-t per
// component and column).  With (alpha [K], m, kappa, a, b [K, D]) = svi/mog.unpack(eta):
//     logit_k(x) = c_k - sum_d h_kd log1p(q_kd (x_d - m_kd)^2)
//         h = a + 1/2,   q = kappa / (2 b (kappa + 1)),
//         c_k = log alpha_k - log sum alpha + sum_d [lnGamma(a + 1/2) - lnGamma(a) + log(q / pi) / 2]
//     lpd(x) = logsumexp_k logit_k(x),   R_k(x) = exp(logit_k(x) - lpd(x)),   label(x) = argmax_k logit_k(x)
// The logit is formed from (x - m)^2, never from the expanded quadratic: on data that are not centred (|x| ~ 170,
// tests/test_mixture_multi_tile_gpu.py) the expanded form is a small difference of terms thousands of times its size.
//
// K D terms per row, each one logarithm and one reciprocal, none of it a contraction: a VALU / transcendental kernel.
//   * one row per lane, its <= 16 columns in registers; a wave owns 64-row tiles;
//   * the table [m | q | h] of a component is uniform over the wave and is read through uniform (scalar) loads: every
//     vector instruction of a term takes at most one of its entries, so none of them costs a vector register;
//   * the loop over k carries a running maximum, sum and argmax (no array of logits: one indexed by the loop counter
//     would live in scratch); with R the logits also go to wave-private LDS as [component][row] and leave, rescaled,
//     as whole rows of R (lane = component: one contiguous store per row).
// log1p(u) is log(w) u / (w - 1) with w = 1 + u (w - 1 is exact, the quotient undoes the rounding of w; w == 1: u
// itself), the form of the Beta link in csrc/bsc_families.h: a well-fitted component has a ~ N_k / 2 (8e4 at config 3's
// size), u ~ z^2 / 2a, and h multiplies whatever log(1 + u) loses -- 6e-3 on a term of 8 at a = 1e5 where this form is
// off by 1.5e-6 (tests/test_mog_predict_cpu.py holds both).
#include "bsc_common.h"

namespace {

constexpr int PK = 64;          // components at most
constexpr int PD = 16;          // data columns at most
constexpr int PT = 64;          // rows per tile: one per lane
constexpr int P_BLOCK = 256;
constexpr int P_WAVES = P_BLOCK / BSC_WAVE;
constexpr int P_WAVES_PER_CU = 16;          // the grid is sized for this many resident waves per CU
constexpr int PR_STRIDE = PT + 1;           // LDS row stride of the logit tile [component][row]: both sides conflict-free
constexpr int P_SUM_BLOCK = 256;

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // X is 4-byte aligned, no more

// No contraction the source does not spell out: the four instantiations below must round alike (a row's lpd and label
// do not depend on which outputs were asked for), and w - 1 undoes w = 1 + u only if that sum is rounded once.
#pragma clang fp contract(off)

// WITH_R: 4 waves x 64 x 65 floats of LDS = 65 KiB a workgroup, two workgroups a CU
template <bool FULL, bool WITH_R>   // FULL: D == 16, no column guards
__global__ __launch_bounds__(P_BLOCK, WITH_R ? 2 : 4) void mog_predict_kernel(
    const float* __restrict__ X, int64_t ldx, int64_t N, int D, int K, const float* __restrict__ Pt,
    const float* __restrict__ cvec, float* __restrict__ lpd, int* __restrict__ label, float* __restrict__ R,
    int64_t ldr, double* __restrict__ slab, int n_iter) {
    __shared__ float rt[WITH_R ? P_WAVES * PK * PR_STRIDE : 1];
    __shared__ double wsum[P_WAVES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
    const int DD = FULL ? PD : D;
    float* const lt = rt + (WITH_R ? wave * PK * PR_STRIDE : 0);

    double acc = 0.0;       // this lane's rows, in tile order
    const int64_t stride = (int64_t)gridDim.x * P_WAVES;
    int64_t tile = (int64_t)blockIdx.x * P_WAVES + wave;
    for (int it = 0; it < n_iter; ++it, tile += stride) {
        const int64_t row0 = tile * PT;
        if (row0 >= N) break;                               // (uniform over the wave; no workgroup barrier in here)
        const int64_t row = row0 + lane;
        const bool valid = row < N;
        // a lane past the end reads the tile's first row again (in bounds, no branch) and stores nothing
        const float* __restrict__ xr = X + (valid ? row : row0) * ldx;
        float x[PD];
        if (FULL) {
#pragma unroll
            for (int c4 = 0; c4 < PD / 4; ++c4) {
                const f32x4u v = *reinterpret_cast<const f32x4u*>(xr + 4 * c4);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[4 * c4 + j] = v[j];
            }
        } else {
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                x[d] = 0.f;
                if (d < D) x[d] = xr[d];                    // columns >= D belong to the next row, or to nobody
            }
        }

        float mx = -3.0e38f, sum = 0.f;
        int arg = 0;
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ p = Pt + (int64_t)k * 3 * DD;      // uniform: [m | q | h] of component k
            float a2 = 0.f;                                 // sum_d h log2(1 + u)
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                if (FULL || d < D) {                        // (uniform guard, constant register index)
                    const float dm = x[d] - p[d];
                    const float u = p[DD + d] * (dm * dm);
                    const float w = 1.0f + u;
                    // log2(w) / (w - 1), log2(e) where w == 1: times u it is log1p(u) / log(2)
                    const float ratio = __builtin_amdgcn_logf(w) * __builtin_amdgcn_rcpf(w - 1.0f);
                    a2 = fmaf(p[2 * DD + d], u * (w == 1.0f ? LOG2E : ratio), a2);
                }
            }
            const float l = fmaf(-LN2, a2, cvec[k]);
            if (WITH_R) lt[k * PR_STRIDE + lane] = l;
            // running maximum, argmax (the lowest index among equal maxima) and sum of exp(l - maximum)
            const bool up = l > mx;
            const float e = __builtin_amdgcn_exp2f(-fabsf(l - mx) * LOG2E);
            sum = up ? fmaf(sum, e, 1.0f) : sum + e;
            arg = up ? k : arg;
            mx = up ? l : mx;
        }
        const float lp = fmaf(LN2, __builtin_amdgcn_logf(sum), mx);    // (sum >= 1)
        if (valid) {
            if (lpd) lpd[row] = lp;
            if (label) label[row] = arg;
            acc += (double)lp;
        }
        if (WITH_R) {
            const float inv = 1.0f / sum;
            const int64_t left = N - row0;
            const int n_rows = __builtin_amdgcn_readfirstlane((int)(left < PT ? left : PT));
            wave_lds_sync();
            for (int r = 0; r < n_rows; ++r) {              // lane = component: a row of R is one contiguous store
                const float mr = readlane_f32(mx, r), ir = readlane_f32(inv, r);
                if (lane < K)
                    R[(row0 + r) * ldr + lane] = __builtin_amdgcn_exp2f((lt[lane * PR_STRIDE + r] - mr) * LOG2E) * ir;
            }
            wave_lds_sync();                                // the next tile overwrites the logits
        }
    }

    if (slab) {     // fixed order: rows of a lane by tile, lanes by the butterfly, waves and then workgroups by index
        const double t = wave_allsum_f64(acc);
        if (lane == 0) wsum[wave] = t;
        __syncthreads();
        if (tid == 0) {
            double b = wsum[0];
#pragma unroll
            for (int w = 1; w < P_WAVES; ++w) b += wsum[w];
            slab[blockIdx.x] = b;
        }
    }
}

// float64, fixed-order sum of the workgroups' partials (n may be 0: the sum of no rows)
__global__ __launch_bounds__(P_SUM_BLOCK) void mog_predict_sum_kernel(const double* __restrict__ slab, int n,
                                                                     double* __restrict__ out) {
    __shared__ double part[P_SUM_BLOCK];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += P_SUM_BLOCK) s += slab[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = P_SUM_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

// eta layout: [alpha-1 (K) | kappa*m (K*D) | kappa (K*D) | 2a-1 (K*D) | 2b+kappa*m^2 (K*D)] (csrc/bsc_mog.hip).
// One workgroup, 16 lanes per component and one column each, 64 components per sweep; a component's D terms are added
// in a fixed butterfly order inside its 16-lane group.  Everything in float64, rounded once.
__global__ __launch_bounds__(1024) void mog_predictive_params_kernel(const double* __restrict__ eta, int K, int D,
                                                                     float* __restrict__ Pt,
                                                                     float* __restrict__ cvec) {
    __shared__ double alpha_sum;
    const int dl = threadIdx.x & 15;
    if (threadIdx.x < 64) {   // one wave: the Dirichlet's total, fixed order
        double a = 0.0;
        for (int j = threadIdx.x; j < K; j += 64) a += eta[j] + 1.0;
        const double tot = wave_allsum_f64(a);
        if (threadIdx.x == 0) alpha_sum = tot;
    }
    __syncthreads();
    const double log_sum = log(alpha_sum);
    const int64_t KD = (int64_t)K * D;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + (threadIdx.x >> 4);
        double cs = 0.0;
        for (int d0 = 0; d0 < D; d0 += 16) {
            const int d = d0 + dl;
            const bool cell = k < K && d < D;
            const int64_t i = cell ? (int64_t)k * D + d : 0;
            const double e1 = eta[K + i], kappa = eta[K + KD + i], e3 = eta[K + 2 * KD + i], e4 = eta[K + 3 * KD + i];
            const double m = e1 / kappa, a = 0.5 * (e3 + 1.0), b = 0.5 * (e4 - kappa * m * m);
            const double q = kappa / (2.0 * b * (kappa + 1.0)), h = a + 0.5;
            const double t = bsc_lgamma_f64(h) - bsc_lgamma_f64(a) + 0.5 * log(q / BSC_PI);
            if (cell) {
                float* row = Pt + (int64_t)k * 3 * D;
                row[d] = (float)m;
                row[D + d] = (float)q;
                row[2 * D + d] = (float)h;
                cs += t;
            }
        }
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) cs += __shfl_xor(cs, off);
        if (k < K && dl == 0) cvec[k] = (float)(log(eta[k] + 1.0) - log_sum + cs);
    }
}

}  // namespace

extern "C" {

int bsc_mog_predictive_params(bsc_ctx* ctx, const double* eta, int32_t K, int32_t D, float* Pt, float* c) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(eta && Pt && c, "bsc_mog_predictive_params: null pointer");
    BSC_REQUIRE(K >= 1 && D >= 1, "bsc_mog_predictive_params: K=%d D=%d", K, D);
    if (K > 1024) return bsc_fail(BSC_ERR_UNSUPPORTED, "bsc_mog_predictive_params: K=%d > 1024 components", K);
    hipLaunchKernelGGL(mog_predictive_params_kernel, dim3(1), dim3(1024), 0, ctx->stream, eta, (int)K, (int)D, Pt, c);
    BSC_LAUNCH_CHECK();
    return BSC_OK;
}

int bsc_mog_predict_pass(bsc_ctx* ctx, const float* X, int64_t ldx, int64_t N, int32_t D, int32_t K, const float* Pt,
                         const float* c, float* lpd, int32_t* label, float* R, int64_t ldr, double* lpd_sum) {
    BSC_CHECK_CTX(ctx);
    BSC_REQUIRE(N >= 0 && ((X != nullptr) || N == 0) && Pt && c, "bsc_mog_predict_pass: null pointer");
    BSC_REQUIRE(lpd || label || R || lpd_sum, "bsc_mog_predict_pass: no output (lpd, label, R and lpd_sum are all NULL)");
    if (D < 1 || D > PD || K < 1 || K > PK)
        return bsc_fail(BSC_ERR_UNSUPPORTED, "bsc_mog_predict_pass: D=%d K=%d outside the fused pass's limits (D<=%d, K<=%d)",
                        D, K, PD, PK);
    BSC_REQUIRE(ldx >= D && ldx < ((int64_t)1 << 25), "bsc_mog_predict_pass: bad ldx=%lld", (long long)ldx);
    BSC_REQUIRE(((uintptr_t)X & 3) == 0, "bsc_mog_predict_pass: X must be 4-byte aligned");
    BSC_REQUIRE(!R || ldr >= K, "bsc_mog_predict_pass: bad ldr=%lld", (long long)ldr);
    // the grid (restated by tests/_mog_predict_ref.py): 64-row tiles, at most P_WAVES_PER_CU waves per CU, every wave
    // the same number of trips
    const int64_t n_tiles = (N + PT - 1) / PT;
    const int64_t max_waves = (int64_t)P_WAVES_PER_CU * ctx->cu_count;
    int n_iter = 0, n_blocks = 0;
    if (n_tiles > 0) {
        const int64_t it = (n_tiles + max_waves - 1) / max_waves;
        const int64_t waves = (n_tiles + it - 1) / it;
        n_iter = (int)it;
        n_blocks = (int)((waves + P_WAVES - 1) / P_WAVES);
    }
    void* ws = nullptr;
    if (lpd_sum) {
        int rc = bsc_workspace(ctx, (size_t)(n_blocks > 0 ? n_blocks : 1) * sizeof(double), &ws);
        if (rc != BSC_OK) return rc;
        ctx->slab_rows = 0;
    }
    if (n_blocks > 0) {
        bsc_prof_scope prof(ctx);
        bsc_with_flags(
            [&](auto full, auto with_r) {
                hipLaunchKernelGGL((mog_predict_kernel<decltype(full)::value, decltype(with_r)::value>), dim3(n_blocks),
                                   dim3(P_BLOCK), 0, ctx->stream, X, ldx, N, (int)D, (int)K, Pt, c, lpd, (int*)label, R, ldr,
                                   (double*)ws, n_iter);
            },
            D == PD, R != nullptr);
    }
    BSC_LAUNCH_CHECK();
    if (lpd_sum) {
        hipLaunchKernelGGL(mog_predict_sum_kernel, dim3(1), dim3(P_SUM_BLOCK), 0, ctx->stream, (const double*)ws, n_blocks,
                           lpd_sum);
        BSC_LAUNCH_CHECK();
    }
    return BSC_OK;
}

}  // extern "C"
