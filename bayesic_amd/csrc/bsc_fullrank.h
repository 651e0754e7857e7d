// The body the full-covariance finishes share (blr_fullrank_update_kernel in csrc/bsc_blr_full.hip,
// glm_fullrank_update_kernel in csrc/bsc_glm_full.hip, glm_scalar_fullrank_update_kernel in
// csrc/bsc_glm_scalar_full.hip): q = N(mu, L L^T) over P parameters, lam = [mu (P) | L packed
// row-major, lower triangle incl. the diagonal], row i at P + i(i+1)/2 with rho_i = log L_ii in its diagonal slot.
// Workgroup k owns rows k and P-1-k of L (k + 1 and P - k entries: equal work); once a kernel's own prologue has put
// g_{s,i} = d f / d z_i at draw s of its rows into LDS, everything below is the same for every model: the gradient
// of mu_i and of the row's entries, Adam on each, and the rows' share of the next draw z' = mu' + L' eps'.  Every sum
// runs in a fixed order and nothing is contracted into FMAs, so that with a diagonal L this is the mean-field
// finish's arithmetic.  Header-only, internal linkage (csrc/bsc_regress.h says why).
#pragma once

#include "bsc_regress.h"

namespace {

constexpr int FR_BLOCK = 256;
constexpr int FR_WAVES = FR_BLOCK / BSC_WAVE;
constexpr int FR_MAX_S = 64;

struct fr_rows {
    int row0, row1;   // row1 >= row0
    int n_rows;       // 1: the middle row of an odd P
};

__device__ __forceinline__ fr_rows fr_row_pair(int k, int P) {
    return fr_rows{k, P - 1 - k, k == P - 1 - k ? 1 : 2};
}

// Gradient + Adam: one entry per thread; item j = -1 is mu_i, j = 0..i the row's entries of L.  Leaves the new rows
// in Lnew (diagonal as e^{rho'}) and mu_new for fr_next_draw.  E: row stride of the noise eps[S, E].
template <int N>
__device__ __forceinline__ void fr_grad_adam(const fr_rows& rp, int P, int E, int S, const double (&gs)[2][FR_MAX_S],
                                             const double* lam_in, double* lam_out, double* am1, double* am2,
                                             double* grad, const double* eps, const bsc_adam& adam,
                                             double (&Lnew)[2][N], double (&mu_new)[2]) {
#pragma clang fp contract(off)
    const double inv_S = 1.0 / (double)S;
    const int n0 = rp.row0 + 2;
    const int n_items = n0 + (rp.n_rows == 2 ? rp.row1 + 2 : 0);
    for (int it = threadIdx.x; it < n_items; it += FR_BLOCK) {
        const int r = it < n0 ? 0 : 1;
        const int i = r ? rp.row1 : rp.row0;
        const int j = (r == 0 ? it : it - n0) - 1;
        const int64_t off = j < 0 ? (int64_t)i : (int64_t)P + (int64_t)i * (i + 1) / 2 + j;
        const double p = lam_in[off];
        double m1 = am1[off], m2 = am2[off];
        double acc = 0.0;
        if (j < 0) {
            for (int s = 0; s < S; ++s) acc += gs[r][s];
        } else {
            for (int s = 0; s < S; ++s) acc += gs[r][s] * eps[(int64_t)s * E + j];
        }
        double g = acc * inv_S;
        if (j == i) g = g * exp(p) + 1.0;
        grad[off] = g;
        const double np = bsc_adam_ascent(p, g, m1, m2, adam);
        am1[off] = m1;
        am2[off] = m2;
        lam_out[off] = np;
        if (j < 0) mu_new[r] = np;
        else Lnew[r][j] = j == i ? exp(np) : np;
    }
}

// Next draw of these rows: z'_{s,i} = mu'_i + sum_{j<=i} L'_ij eps'_sj (a wave per sample, both rows at once);
// store(s, i, z) puts it where row i of the model lives.  Call behind a __syncthreads() after fr_grad_adam.
template <int N, typename Store>
__device__ __forceinline__ void fr_next_draw(const fr_rows& rp, int E, int S, const double* eps_next,
                                             const double (&Lnew)[2][N], const double (&mu_new)[2], Store store) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = wave; s < S; s += FR_WAVES) {
        const double* e = eps_next + (int64_t)s * E;
        double z0 = 0.0, z1 = 0.0;
        for (int j = lane; j <= rp.row1; j += BSC_WAVE) {
            const double ev = e[j];
            if (j <= rp.row0) z0 += Lnew[0][j] * ev;
            z1 += Lnew[rp.n_rows - 1][j] * ev;
        }
        z0 = wave_allsum_f64(z0);
        z1 = wave_allsum_f64(z1);
        if (lane == 0) {
            store(s, rp.row0, mu_new[0] + z0);
            if (rp.n_rows == 2) store(s, rp.row1, mu_new[1] + z1);
        }
    }
}

// ---- host side: what the entry points check and do alike ----------------------------------------------------------

// The state and size checks (the next-draw buffers and the noise: next_draw_noise, csrc/bsc_regress.h);
// `stats_layout` names the data pass's statistics ("Q | G", "ell | G").
inline int fr_check_state(const char* who, const char* stats_layout, const double* stats, bool pointers_set,
                          const double* lam_in, const double* lam_out, int32_t D, int max_d, int32_t S, int64_t t) {
    BSC_REQUIRE(stats, "%s: stats must be the [%s] of the data pass (pending partials are not read)", who,
                stats_layout);
    BSC_REQUIRE(pointers_set, "%s: null pointer", who);
    BSC_REQUIRE(lam_in != lam_out, "%s: lam_in and lam_out must differ", who);
    BSC_REQUIRE(D >= 4 && D <= max_d && D % 4 == 0, "%s: D=%d must be a multiple of 4 in [4,%d]", who, D, max_d);
    BSC_REQUIRE(S >= 1 && S <= FR_MAX_S, "%s: S=%d must be in [1,%d]", who, S, FR_MAX_S);
    BSC_REQUIRE(t >= 1, "%s: the Adam step count starts at 1", who);
    return BSC_OK;
}

}  // namespace
