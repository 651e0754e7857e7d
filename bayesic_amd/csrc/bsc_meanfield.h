// The two-launch mean-field finish of the models whose latent is z = [w (D) | the model's own coordinates]: the bodies
// of glm_hier_scalars_kernel / glm_hier_coord_kernel (csrc/bsc_glm_group.hip) and scalar_mf_scalars_kernel /
// scalar_mf_coord_kernel (csrc/bsc_scalar_family.h).  q = N(m, diag e^{2 rho}), lam = [m (P) | rho (P)], eps [S, P].
//
//   scalars  workgroup s < S: |w_s|^2 and what else the model keeps per draw, into scal; workgroup S: sum rho.
//   coord    one thread per coordinate i of z: d f / d z_i over the draws in draw order, the entropy term, Adam on m_i
//            and rho_i, the ELBO in thread P - 1, the coordinate's next draws.
//
// A Model is the arguments (MeanfieldArgs plus its own fields) with these static members:
//   N_SLOTS                   runs of MF_MAX_S doubles it keeps in scal; f_s = scale ell_s + log p(z_s) is the last
//                             one, sum rho sits behind it
//   LAST_HAS_NEXT             whether coordinate P - 1 has a next draw to store
//   extra_sq(a, s, red)       one more block sum the per-draw scalars need (all threads; 0.0 for none)
//   draw_scalars(a, s, wsq, xsq)   thread 0 of workgroup s: fills scal[k * MF_MAX_S + s]
//   grad_term(a, i, s)        d f / d z_i at draw s for a coordinate i >= D
//   store_next(a, i, nm, sd)  the next draws of a coordinate i >= D, mean nm and standard deviation sd
// The w coordinates (prior N(0, I / prec), statistics G behind ell in stats, draws W [S, D]) are the same for every
// model and live here.  Header-only, internal linkage (csrc/bsc_regress.h says why); nothing but bsc_adam_ascent sets a
// contraction mode, as in the kernels this came out of.
#pragma once

#include "bsc_regress.h"

namespace {

constexpr int MF_BLOCK = 256;
constexpr int MF_WAVES = MF_BLOCK / BSC_WAVE;
constexpr int MF_MAX_S = 64;

struct MeanfieldArgs {
    const double* stats;     // [ell (S) | G (S D) | the model's]
    const double* lam_in;
    double* lam_out;
    double* m1;
    double* m2;
    const double* eps;       // [S, P]
    const float* W;          // [S, D]
    const double* eps_next;  // nullptr: no next draw
    float* W_next;
    double* scal;            // [N_SLOTS][MF_MAX_S] | sum rho
    double* elbo;
    double* grad;
    int D, S, P;
    double scale, prec, a0, b0;
    double c0;               // the terms of log p(z) free of z
    bsc_adam adam;
};

// the block's sum of one value per thread: waves in wave order
template <int WAVES>
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_allsum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int k = 1; k < WAVES; ++k) t += red[k];
    __syncthreads();
    return t;
}

template <class Model>
__device__ __forceinline__ void meanfield_scalars_body(const Model& a) {
    __shared__ double red[MF_WAVES];
    const int tid = threadIdx.x;
    const int D = a.D, S = a.S, P = a.P;
    const int s = (int)blockIdx.x;
    if (s == S) {
        double part = 0.0;
        for (int i = tid; i < P; i += MF_BLOCK) part += a.lam_in[P + i];
        const double t = block_sum_f64<MF_WAVES>(part, red);
        if (tid == 0) a.scal[Model::N_SLOTS * MF_MAX_S] = t;
        return;
    }
    double pw = 0.0;
    for (int d = tid; d < D; d += MF_BLOCK) {
        const double wv = (double)a.W[(int64_t)s * D + d];
        pw += wv * wv;
    }
    const double wsq = block_sum_f64<MF_WAVES>(pw, red);
    const double xsq = Model::extra_sq(a, s, red);
    if (tid == 0) Model::draw_scalars(a, s, wsq, xsq);
}

template <class Model>
__device__ __forceinline__ void meanfield_coord_body(const Model& a) {
    const int D = a.D, S = a.S, P = a.P;
    const int i = blockIdx.x * MF_BLOCK + threadIdx.x;
    if (i >= P) return;
    const double* G = a.stats + S;
    double gm = 0.0, gr = 0.0;
    for (int s = 0; s < S; ++s) {
        const double g = i < D ? a.scale * G[(int64_t)s * D + i] - a.prec * (double)a.W[(int64_t)s * D + i]
                               : Model::grad_term(a, i, s);
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
        for (int s = 0; s < S; ++s) fsum += a.scal[(Model::N_SLOTS - 1) * MF_MAX_S + s];
        a.elbo[0] = fsum * inv_S + a.scal[Model::N_SLOTS * MF_MAX_S] + 0.5 * (double)P * (1.0 + BSC_LOG_2PI);
        if (!Model::LAST_HAS_NEXT) return;
    }
    if (!a.eps_next) return;
    const double sd = exp(nr);
    if (i < D) {
        for (int s = 0; s < S; ++s) a.W_next[(int64_t)s * D + i] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
    } else {
        Model::store_next(a, i, nm, sd);
    }
}

// ---- the model with ONE scalar behind the weights whose exponential has a Gamma(a0, b0) prior ------------------------
//
// z = [w (D) | tau]: the negative binomial's dispersion phi = e^tau (csrc/bsc_glm_nb.hip) and the Gamma likelihood's
// shape alpha = e^tau (csrc/bsc_glm_gamma.hip).  The likelihood enters through ell_s, G_s and T_s = d ell_s / d tau_s
// alone, so the finish is the same for both and each translation unit instantiates the bodies above with this model.
// scal = [g_tau (64) | f (64) | sum rho]; c0 = D/2 log(prec / 2 pi) + a0 log b0 - lnGamma(a0).
struct NbModel : MeanfieldArgs {
    const float* logphi;     // [S]
    float* logphi_next;

    static constexpr int N_SLOTS = 2;
    static constexpr bool LAST_HAS_NEXT = true;

    static __device__ __forceinline__ double extra_sq(const NbModel&, int, double*) { return 0.0; }

    // g_tau and f_s = scale ell_s + log p(z_s) with tau_s the float32 value the pass read; T sits behind G in stats
    static __device__ __forceinline__ void draw_scalars(const NbModel& a, int s, double wsq, double) {
        const int D = a.D, S = a.S;
        const double tau = (double)a.logphi[s];
        const double phi = exp(tau);
        const double T = a.stats[S + (int64_t)S * D + s];
        a.scal[s] = a.scale * T + a.a0 - a.b0 * phi;
        a.scal[MF_MAX_S + s] = a.scale * a.stats[s] + a.c0 - 0.5 * a.prec * wsq + a.a0 * tau - a.b0 * phi;
    }

    static __device__ __forceinline__ double grad_term(const NbModel& a, int, int s) { return a.scal[s]; }

    static __device__ __forceinline__ void store_next(const NbModel& a, int i, double nm, double sd) {
        const int S = a.S, P = a.P;
        for (int s = 0; s < S; ++s) a.logphi_next[s] = (float)(nm + sd * a.eps_next[(int64_t)s * P + i]);
    }
};

// (The kernels and the host side of that finish: csrc/bsc_scalar_family.h, scalar_family_update.)

}  // namespace
