// The bodies of the GLM training-pass kernels (csrc/bsc_glm.hip's header comment describes the two tile shapes), as
// __device__ templates with one compile-time flag so that two translation units can instantiate them:
//
//   OBS = false   csrc/bsc_glm.hip: glm_pass_kernel / glm_pass_mfma_kernel, the pass over (X, y) alone.  Every use of
//                 the offset and the weight is behind `if (OBS)`, the tile structs carry no extra registers, and the
//                 kernels come out as they did when the bodies lived in that file.
//   OBS = true    csrc/bsc_glm_obs.hip: glm_obs_pass_kernel / glm_obs_pass_mfma_kernel, with a per-row offset o_n
//                 (added to the logit before the link) and a per-row weight v_n >= 0:
//                     l[n,s] = x_n . w_s + o[n],  ell[s] = sum_n v[n] (y[n] l[n,s] - A(l[n,s])),
//                     G[s,:] = sum_n v[n] (y[n] - A'(l[n,s])) x_n
//                 A row with v_n = 0 adds exactly nothing, by a select and not by a product (its link value may have
//                 overflowed).  o and v ride in the tile struct next to y and are loaded the way y is; a null offset
//                 is a zero-record descriptor (reads 0, costs nothing), a null weight a uniform select of 1.0f.
//                 Rows past B read o = 0 and v = 0 through the descriptors.
//   GRP = true    csrc/bsc_glm_group.hip (always with OBS): a per-row group id g_n and one intercept per (group, draw),
//                     l[n,s] = x_n . w_s + Bz[g_n][s] + o[n]
//                 The id rides in the tile next to y (rows past B read id 0); the intercept is gathered through a
//                 descriptor of exactly J * 32 bytes -- no id can read outside the table -- BEFORE the forward
//                 contraction and before the next tile's loads are issued (loads return in order: behind them the
//                 gather would wait for the whole prefetch).  Besides the slab the pass leaves every residual
//                 r_ns = v_n (y_n - A'(l_ns)) in a workspace R, 32 bytes per row in 16-row blocks [block][draw][row],
//                 through a descriptor over what is left of R from the tile's block on: the tail tiles of n_iter run
//                 past the batch and their stores do not land.  Everything of it is behind `if constexpr (GRP)`; the
//                 flag defaults to off and the kernels of the two files above compile as they did without it.
//
//                 GRP with DSP (csrc/bsc_glm_scalar_group.hip): the link of the GRP branches also gets the draw's
//                 dispersion and the T accumulator, the slab is DSP's; never with ITV.
//
//   DSP = true    csrc/bsc_glm_nb.hip (always with OBS and LINK = GLM_NEGBIN): the negative binomial with one
//                 dispersion draw per weight draw, tau_s = log phi_s as float32 [S].  A lane owns ONE draw in both tile
//                 shapes, so tau_s, phi_s = exp(tau_s), lnGamma(phi_s) and psi(phi_s) are made once per launch (the two
//                 special values in float64, then rounded) and stay in four registers; T[s] = d ell[s] / d tau_s is one
//                 more lane accumulator next to ell.  The slab has no room for it, so these kernels write block
//                 partials of NB_SLAB_STRIDE = REG_SLAB_G + 16 floats: ell at [SLAB_G + s], T at [SLAB_G + 8 + s].
//                 Everything of it is behind `if constexpr (DSP)`; the flag defaults to off.
//                 csrc/bsc_glm_gamma.hip (LINK = GLM_GAMMA) runs the same flag with a shape alpha_s = exp(tau_s) in the
//                 place of phi_s: the four registers are tau_s, alpha_s and the two per-draw constants of the Gamma
//                 density (glm_link below), T[s] and the slab are the same.
//                 csrc/bsc_glm_weibull.hip (LINK = GLM_WEIBULL) runs it with the Weibull shape k_s = exp(tau_s): only
//                 tau_s and k_s are kept (the density has no per-draw constant), and the censoring flag of a row is
//                 the sign of its y, so the tiles carry nothing new.
//                 csrc/bsc_glm_beta.hip (LINK = GLM_BETA) runs it with the Beta precision phi_s = exp(tau_s): the four
//                 registers are the negative binomial's (tau_s, phi_s, lnGamma(phi_s), psi(phi_s)); lnGamma and psi at
//                 m phi and (1 - m) phi are float32, per (row, draw) (csrc/bsc_special_f32.h, bsc_lgamma_psi_f32).
//   ITV = true    csrc/bsc_glm_weibull_interval.hip (always with DSP and LINK = GLM_WEIBULL): interval and left
//                 censoring.  One more per-row vector, `upper` [B] float32, rides in the tiles next to y and is loaded
//                 the way y is (rows past B read 0); glm_link says how it is read.  Everything of it is behind
//                 `if constexpr (ITV)`; the flag defaults to off and every other kernel compiles as it did.
//
// Header-only, internal linkage, like csrc/bsc_regress.h.
#pragma once

#include "bsc_regress.h"
#include "bsc_special_f32.h"

namespace {

constexpr int SLAB_G = REG_SLAB_G;            // slab[b][d*8 + s], then ell at [SLAB_G + s]
constexpr int SLAB_STRIDE = REG_SLAB_STRIDE;  // floats per block partial
constexpr int NB_SLAB_STRIDE = REG_SLAB_G + 2 * SG;   // DSP: ell at [SLAB_G + s], T at [SLAB_G + 8 + s]
constexpr int GLM_NEGBIN = 2;                 // the third link; internal: the BSC_GLM_* entry points refuse it
constexpr int GLM_GAMMA = 3;                  // the fourth, internal as well: csrc/bsc_glm_gamma.hip
constexpr int GLM_WEIBULL = 4;                // the fifth, internal as well: csrc/bsc_glm_weibull.hip
constexpr int GLM_BETA = 5;                   // the sixth, internal as well: csrc/bsc_glm_beta.hip

// DSP: what a lane keeps of its draw's dispersion (GLM_GAMMA: of its draw's shape alpha_s; GLM_WEIBULL: of k_s;
// GLM_BETA: of its draw's precision phi_s).
struct GlmDisp {
    float tau, phi;     // log phi_s as the pass read it, exp(tau)
    float lg, psi;      // lnGamma(phi), psi(phi) (GLM_NEGBIN and GLM_BETA); GLM_GAMMA: c_a = alpha log alpha -
                        // lnGamma(alpha), c_1 = log alpha + 1 - psi(alpha); GLM_WEIBULL: not used (0)
};

// Draw s of this launch's chunk (s >= S: a dead slot, phi = 1).  The special values in float64, once per launch.
template <int LINK = GLM_NEGBIN>
__device__ __forceinline__ GlmDisp glm_disp_of(const float* __restrict__ logphi, int s, int S) {
    GlmDisp d;
    d.tau = s < S ? logphi[s] : 0.0f;
    d.phi = expf(d.tau);
    if constexpr (LINK == GLM_WEIBULL) {
        d.lg = d.psi = 0.0f;       // tau and k alone: the Weibull density has no special function in it
    } else if constexpr (LINK == GLM_GAMMA) {
        const double a = (double)d.phi, la = log(a);
        d.lg = (float)(a * la - bsc_lgamma_f64(a));
        d.psi = (float)(la + 1.0 - bsc_digamma_f64(a));
    } else {                       // GLM_NEGBIN and GLM_BETA: lnGamma(phi) and psi(phi) themselves
        d.lg = (float)bsc_lgamma_f64((double)d.phi);
        d.psi = (float)bsc_digamma_f64((double)d.phi);
    }
    return d;
}

// ---- the link: ell += y l - A(l) for a real row, resid = y - A'(l) ------------------------------------------
//
// Logistic: A = softplus in the stable form max(l, 0) + log1p(e), e = exp(-|l|) <= 1 (exp at full float32 accuracy:
// the tails at |l| = 80 are compared at rtol 1e-6), and A' = sigmoid from the
// same e (1 / (1 + e) for l >= 0, e / (1 + e) below): finite for every finite l.  Poisson: A = A' = exp(l),
// NOT clamped (a clamp would change the gradient silently): finite for l <= 88.
// OBS: `l` already holds the offset; both terms are scaled by the weight vv where vv > 0 and are exactly 0 elsewhere.
// GLM_NEGBIN (always OBS; dp and T set): with u = l - tau, phi = e^tau, z = y + phi and the logistic forms at u,
//     ell  += v [ dlnGamma(y, phi) + y u - z softplus(u) ]          dlnGamma = lnGamma(z) - lnGamma(phi)
//     resid = v [ y - z sigmoid(u) ]                                                           (= d / d l)
//     T    += v [ phi dpsi(y, phi) - phi softplus(u) ] - resid       dpsi = psi(z) - psi(phi)   (= d / d tau)
// finite for every finite l; both differences are exactly 0 at y = 0 (csrc/bsc_special_f32.h: an empty product).
// GLM_GAMMA (always OBS; dp and T set): y > 0, alpha = e^tau, ly = log y, q = y e^{-l}, and dp's c_a, c_1:
//     ell  += v [ c_a + alpha (ly - l - q) - ly ]                    (the full density, nothing left out)
//     resid = v alpha (q - 1)                                                                  (= d / d l)
//     T    += v alpha (c_1 + ly - l - q)                                                       (= d / d tau)
// NOT clamped, like the Poisson link: finite while e^{-l} and y e^{-l} are below the float32 maximum (l > -88 at
// y = 1).  One exp and one log per (row, draw), both at full float32 accuracy: ly enters ell multiplied by alpha.
// GLM_WEIBULL (always OBS; dp and T set): the sign of y is the censoring flag -- y > 0 an event at y, y < 0 right-censored
// at -y -- so delta = (y > 0), t = |y|; k = e^tau, ly = log t, z = k (ly - l), l the log SCALE:
//     ell  += v [ delta (tau + z - ly) - e^z ]            (log f = tau + z - ly - e^z, log S = -e^z: nothing left out)
//     resid = v k (e^z - delta)                                                                (= d / d l)
//     T    += v [ delta (1 + z) - z e^z ]                                                      (= d / d tau)
// NOT clamped, like the Poisson and Gamma links: finite while z stays below about 88 (e^z and z e^z below the float32
// maximum).  One log and one exp per (row, draw) at full float32 accuracy; z is rounded before the exponential, which
// costs |z| eps of e^z (the tests' bounds count (1 + |z|) e^z per row).  y = 0 or a non-finite y on a kept row is the
// caller's to keep out.
// GLM_BETA (always OBS; dp and T set): 0 < y < 1, phi = e^tau, ly = log y, l1y = log1p(-y), m = sigmoid(l) and
// 1 - m = sigmoid(-l) EACH from the stable logistic forms e / (1 + e), 1 / (1 + e) with e = exp(-|l|) (never 1 - m by
// subtraction), a = m phi, b = (1 - m) phi, and dp's lnGamma(phi), psi(phi):
//     ell  += v [ lnGamma(phi) - lnGamma(a) - lnGamma(b) + (a - 1) ly + (b - 1) l1y ]    (the full density, nothing left out)
//     resid = v phi m (1 - m) [ (ly - l1y) - psi(a) + psi(b) ]                                (= d / d l)
//     T    += v phi [ psi(phi) + m (ly - psi(a)) + (1 - m)(l1y - psi(b)) ]                     (= d / d tau)
// lnGamma and psi of a and of b from csrc/bsc_special_f32.h's bsc_lgamma_psi_f32, one evaluation after the other: four
// logs, four reciprocals and two shifted products per (row, draw) on top of the logistic link's exp.  l1y through
// log(w) (-y) / (w - 1), w = 1 - y, which undoes the rounding of w (y = 1e-6: log(1 - y) alone is 6 % off).  NOT
// clamped: finite while a, b and their reciprocals are normal float32 values -- |l| <= 80 at tau in [-2, 5], where
// psi(a) ~ -1 / a reaches 4e35 and is multiplied by m before anything else.  y = 0, y = 1 or a non-finite y on a kept
// row is the caller's to keep out.
// GLM_WEIBULL with ITV (csrc/bsc_glm_weibull_interval.hip): `uv` is the row's entry of the vector `upper` -- 0: the row is
// what y says, as above; uv > 0 (with y < 0): interval-censored on (a, b] = (-y, uv]; uv < 0: left-censored at b = -uv,
// the magnitude of y not read.  With z = k (log a - l), E = e^z, d = log b - log a and Delta = E expm1(k d) = E_b - E_a
// (a left-censored row: z = k (log b - l), Delta = E, and E_a = 0 in what follows), e = e^{-Delta}, p = -expm1(-Delta):
// (d through log1p((b - a) / a) where b < 2 a: the difference of two rounded logarithms would lose a narrow interval)
//     ell  += v [ -E_a + log p ]                                       (= log(S(a) - S(b)): nothing left out)
//     resid = v k ( E_a - Delta e / p )                                (Delta e / p = Delta / expm1(Delta), in (0, 1))
//     T    += v [ -z E_a + (z Delta + k d E_b) e / p ]                 E_b = E_a + Delta
// all three in ONE form with the rows above: an indicator `ic` (1 on such a row, else 0) multiplies the new terms, which
// a row without an upper end evaluates at Delta = 1, k d = 0.  OVERFLOW: where Delta >= ITV_BIG -- e^{-Delta} is zero in
// float32 (csrc/bsc_special_f32.h), or the upper end is so far out that e^{k d} or Delta is infinite (upper = 1e30 for "no bound") -- the row is
// the right-censored one at a (the left-censored one adds nothing: its probability is 1), by the same select on the
// inputs; a NaN Delta (0 times infinity) goes the same way.  Seven transcendentals per (row, draw) for two.

template <int LINK, bool OBS = false, bool ITV = false>
__device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv = 1.0f,
                                          const GlmDisp* dp = nullptr, float* T = nullptr, float uv = 0.0f) {
    static_assert(!ITV || LINK == GLM_WEIBULL, "the upper end belongs to the Weibull link");
    if constexpr (LINK == GLM_WEIBULL && ITV) {
        // The selects sit on the INPUTS, as below: a dropped row is evaluated at a = b = 1, l = 0, delta = 0, ic = 0.
        // Each select is flat, between values at hand: a nested one (keep ? (left ? .. : ..) : ..) comes out as a branch
        // that the logit's last additions sink into, which splits the loop body and spills 150 bytes per lane.
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const bool left = keep && uv < 0.0f;
        const bool itv = keep && uv > 0.0f;
        const float tq = keep ? fabsf(uv < 0.0f ? uv : yv) : 1.0f;     // one select after the other, not nested
        const float bq = itv ? uv : tq;
        const float dl = (keep && uv == 0.0f && yv > 0.0f) ? 1.0f : 0.0f;
        const float lq = keep ? l : 0.0f;
        const float ly = logf(tq);
        const float z = dp->phi * (ly - lq);
        const float ez = expf(z);
        const float kd = dp->phi * bsc_logratio_f32(bq, tq, ly);   // exactly 0 unless the row is an interval
        const float dlt = ez * (bsc_expm1_f32(kd) + (left ? 1.0f : 0.0f));   // expm1(0) = 0 on a left-censored row
        const bool on = (left || itv) && dlt < ITV_BIG;      // false for a NaN as well
        const float ic = on ? 1.0f : 0.0f;
        const float dq = on ? dlt : 1.0f;
        const float kq = on ? kd : 0.0f;
        const float ea = left ? 0.0f : ez;
        const float p = -bsc_expm1_f32(-dq);
        const float q = expf(-dq) * __builtin_amdgcn_rcpf(p);                      // 1 / expm1(Delta), never through an infinite expm1
        const float eb = ea + dq;
        ell = fmaf(vq, fmaf(dl, (dp->tau + z) - ly, fmaf(ic, logf(p), -ea)), ell);
        *T = fmaf(vq, fmaf(dl, 1.0f + z, fmaf(ic * q, fmaf(z, dq, kq * eb), -z * ea)), *T);
        return vq * (dp->phi * (ea - fmaf(ic * q, dq, dl)));
    }
    if constexpr (LINK == GLM_NEGBIN) {
        // The selects sit on the INPUTS: a dropped row (weight 0, or past B) is evaluated at y = 0, u = 0 -- finite
        // whatever it held -- and its terms are multiplied by an exact 0.  A select on the results turns into a
        // branch around the whole evaluation, which splits the loop body and spills.
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.0f;
        const float u = keep ? l - dp->tau : 0.0f;
        const float e = expf(-fabsf(u));
        const float t = 1.0f + e;
        const float r = __builtin_amdgcn_rcpf(t);
        const float sig = u >= 0.0f ? r : e * r;
        // log1p(e) from the full-accuracy log and a true division: softplus is multiplied by y + phi and the products
        // cancel against lnGamma(y + phi) and y u, so the 3e-7 of the logistic link's fast form would show in ell
        // (t == 1: log(t) = 0 and the quotient is over 1, e itself is added -- selects between values at hand)
        const bool tiny = t == 1.0f;
        const float lp = logf(t) * (e / (tiny ? 1.0f : t - 1.0f)) + (tiny ? e : 0.0f);
        const float sp = fmaxf(u, 0.0f) + lp;
        const float z = yq + dp->phi;
        float dlg, dps;                                  // exactly 0 at y = 0
        bsc_dlgamma_dpsi_f32(yq, dp->phi, dp->lg, dp->psi, dlg, dps);
        const float res = fmaf(-z, sig, yq);
        ell = fmaf(vq, dlg + fmaf(yq, u, -z * sp), ell);
        *T = fmaf(vq, fmaf(dp->phi, dps - sp, -res), *T);
        return vq * res;
    }
    if constexpr (LINK == GLM_GAMMA) {
        // The selects sit on the INPUTS, for the reason given above: a dropped row is evaluated at y = 1, l = 0 -- every
        // term finite, log 0 never formed -- and multiplied by an exact 0.
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 1.0f;
        const float lq = keep ? l : 0.0f;
        const float ly = logf(yq);
        // y e^{-l} as a product: expf(ly - l) would round its argument, 4e-6 of the result at |l| = 80.  The difference
        // ly - l is used in the linear term alone.
        const float q = yq * expf(-lq);
        const float d = (ly - lq) - q;
        ell = fmaf(vq, fmaf(dp->phi, d, dp->lg) - ly, ell);
        *T = fmaf(vq, dp->phi * (dp->psi + d), *T);
        return vq * (dp->phi * (q - 1.0f));
    }
    if constexpr (LINK == GLM_BETA) {
        // The selects sit on the INPUTS, for the reason given above: a dropped row is evaluated at y = 1/2, l = 0 -- a = b
        // = phi / 2, every term finite whatever y and l held -- and multiplied by an exact 0.  Each select is flat.
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.5f;
        const float lq = keep ? l : 0.0f;
        const float e = expf(-fabsf(lq));
        const float r = __builtin_amdgcn_rcpf(1.0f + e);
        const float er = e * r;
        const bool pos = lq >= 0.0f;
        const float m = pos ? r : er, m1 = pos ? er : r;         // sigmoid(l) and sigmoid(-l), neither by subtraction
        const float ly = logf(yq);
        const float w = 1.0f - yq;
        const bool one = w == 1.0f;                              // (w - 1 is exact; w == 1: -y itself)
        const float l1y = fmaf(logf(w), yq * __builtin_amdgcn_rcpf(one ? 1.0f : 1.0f - w), one ? -yq : 0.0f);
        const float a = m * dp->phi, b = m1 * dp->phi;
        float lga, psa, lgb, psb;
        bsc_lgamma_psi_f32(a, lga, psa);
        bsc_lgamma_psi_f32(b, lgb, psb);
        ell = fmaf(vq, ((dp->lg - lga) - lgb) + fmaf(a - 1.0f, ly, (b - 1.0f) * l1y), ell);
        *T = fmaf(vq, dp->phi * (dp->psi + fmaf(m, ly - psa, m1 * (l1y - psb))), *T);
        return vq * ((dp->phi * (er * r)) * (((ly - l1y) - psa) + psb));
    }
    if constexpr (LINK == GLM_WEIBULL) {
        // The selects sit on the INPUTS, for the reason given above: a dropped row is evaluated at t = 1, l = 0,
        // delta = 0 -- z = 0, every term finite whatever y held (0 and NaN included) -- and multiplied by an exact 0.
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float tq = keep ? fabsf(yv) : 1.0f;
        const float dl = (keep && yv > 0.0f) ? 1.0f : 0.0f;
        const float lq = keep ? l : 0.0f;
        const float ly = logf(tq);
        const float z = dp->phi * (ly - lq);
        const float ez = expf(z);
        ell = fmaf(vq, fmaf(dl, (dp->tau + z) - ly, -ez), ell);
        *T = fmaf(vq, fmaf(dl, 1.0f + z, -z * ez), *T);
        return vq * (dp->phi * (ez - dl));
    }
    float a, da;
    if (LINK == BSC_GLM_LOGISTIC) {
        const float e = expf(-fabsf(l));
        const float t = 1.0f + e;
        const float r = __builtin_amdgcn_rcpf(t);
        da = l >= 0.0f ? r : e * r;
        // log1p(e) = log(t) e / (t - 1): the quotient undoes the rounding of t = 1 + e (t - 1 is exact); t == 1: e itself.
        // Within 3e-7 of log1p over e in [0, 1], ten vector instructions where the library's log1pf is ~90.
        const float lp = t == 1.0f ? e : __logf(t) * e * __builtin_amdgcn_rcpf(t - 1.0f);
        a = fmaxf(l, 0.0f) + lp;
    } else {
        a = expf(l);
        da = a;
    }
    if (OBS) {
        const bool on = vv > 0.0f;
        ell += (real_row && on) ? vv * fmaf(yv, l, -a) : 0.0f;
        return on ? vv * (yv - da) : 0.0f;
    }
    ell += real_row ? fmaf(yv, l, -a) : 0.0f;
    return yv - da;
}

// ---- 8-row tiles on the VALU (any D % 4 == 0 up to 256): blr_pass_kernel<., 8, .>'s tile (csrc/bsc_regress.h) ----
constexpr int ROWS = 8;
using G8 = Geo<ROWS>;

template <bool OBS, bool GRP = false, bool ITV = false>
struct GlmTile : RowTile<ROWS> {};
template <>
struct GlmTile<true, false, false> : RowTile<ROWS> {
    float ov, vv;   // offset and weight of row lane_value(lane) >> 3, as yv
};
template <>
struct GlmTile<true, false, true> : RowTile<ROWS> {
    float ov, vv;
    float uv;       // ITV: the upper end of the same row (glm_link says how it is read)
};
template <>
struct GlmTile<true, true, false> : RowTile<ROWS> {
    float ov, vv;
    int gv;         // group id of the same row
    float bz;       // Bz[gv][lane_value(lane) & 7], gathered by gather_tile
};

// What the GRP bodies need besides the pass's own arguments (unused, and never touched, without the flag).
struct GlmGroupArgs {
    const int* g;        // [B] group ids, each in [0, J) (checked where the plan is built)
    const float* Bz;     // [J][8]: this launch's chunk of the intercept draws
    int J;
    float* R;            // residuals, [r_blocks][8][16]
    int64_t r_blocks;    // ceil(B / 16)
};
constexpr int R_BLOCK = 16 * SG;   // floats per 16-row block of R

// The intercept table: exactly J records of 32 bytes.  The whole offset of a gather goes into the per-lane operand,
// which is the one the range check covers.
__device__ __forceinline__ auto glm_bz_rsrc(const GlmGroupArgs& ga) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ga.Bz, 0, (unsigned)ga.J * 32u, 0x00020000);
}

// One tile = ROWS rows from row0 on, through descriptors that cover exactly the rows [row0, B).
template <bool FULL, bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void load_tile(GlmTile<OBS, GRP, ITV>& t, const float* __restrict__ X, int64_t ldx,
                                          const float* __restrict__ y, const float* __restrict__ o,
                                          const float* __restrict__ v_, int64_t row0, int64_t B, int D, int lane,
                                          const int* __restrict__ g_ = nullptr,
                                          const float* __restrict__ u_ = nullptr) {
    auto xs = bsc_rows_rsrc(X, ldx, D, B, row0);
    auto ys = bsc_vec_rsrc(y, B, row0);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, 2);   // non-temporal: X is read once
        float4 f = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                               __uint_as_float(v[3]));
        if (!FULL && 4 * lane >= D) f = make_float4(0.f, 0.f, 0.f, 0.f);  // the next row's bytes
        t.x[r] = f;
    }
    t.yv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(ys, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    if constexpr (OBS) {   // a null vector: no records, every lane reads 0
        auto os = bsc_vec_rsrc(o, o ? B : 0, row0);
        auto vs = bsc_vec_rsrc(v_, v_ ? B : 0, row0);
        t.ov = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(os, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
        t.vv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vs, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    }
    if constexpr (GRP) {
        auto gs = bsc_vec_rsrc(g_, B, row0);
        t.gv = (int)__builtin_amdgcn_raw_buffer_load_b32(gs, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0);
    }
    if constexpr (ITV) {   // rows past B read 0: what y says, and y is dropped there
        auto us = bsc_vec_rsrc(u_, B, row0);
        t.uv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(us, 4 * (lane_value<ROWS>(lane) >> 3), 0, 0));
    }
}

// GRP: the intercept of this lane's (row, draw), requested before the next tile's loads are issued.
__device__ __forceinline__ void gather_tile(GlmTile<true, true>& t, const GlmGroupArgs& ga, int lane) {
    t.bz = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
        glm_bz_rsrc(ga), 32 * t.gv + 4 * (lane_value<ROWS>(lane) & 7), 0, 0));
}

// Forward + link + backward for one tile; `wl` is this wave's LDS region, `rows_left` = B - row0.  has_v: the weights
// are set (uniform; without them every row weighs 1.0f and real_row alone masks the rows past B).
// GRP: `row0` is the tile's first row (a multiple of 8), its residuals also go to ga.R.
// DSP: `dp` is the dispersion of this lane's draw, `T` its accumulator.
template <int LINK, bool OBS, bool GRP = false, bool DSP = false, bool ITV = false>
__device__ __forceinline__ void compute_tile(const GlmTile<OBS, GRP, ITV>& t, const float4 (&w)[SG], float4 (&acc)[SG],
                                             float& ell, float* wl, int lane, int64_t rows_left, bool has_v,
                                             const GlmGroupArgs* ga = nullptr, int64_t row0 = 0,
                                             const GlmDisp* dp = nullptr, float* T = nullptr) {
    // 1. per-lane partial dots, row by row, into this lane's row of the buffer
    float* mine = wl + lane * G8::PSTR;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        float4 lo, hi;
        lo.x = dot4(t.x[r], w[0]); lo.y = dot4(t.x[r], w[1]);
        lo.z = dot4(t.x[r], w[2]); lo.w = dot4(t.x[r], w[3]);
        hi.x = dot4(t.x[r], w[4]); hi.y = dot4(t.x[r], w[5]);
        hi.z = dot4(t.x[r], w[6]); hi.w = dot4(t.x[r], w[7]);
        *reinterpret_cast<float4*>(mine + r * SG) = lo;
        *reinterpret_cast<float4*>(mine + r * SG + 4) = hi;
    }
    wave_lds_sync();
    // 2. lane k sums values 4g..4g+3 (g = k % 16) over the lane-rows 16 q .. 16 q + 15
    const int g = lane & (G8::NGRP - 1), q = lane / G8::NGRP;
    const float* col = wl + q * G8::RPQ * G8::PSTR + 4 * g;
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int part = 0; part < G8::RPQ / 8; ++part) {
        float4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float4*>(col + (8 * part + i) * G8::PSTR);
#pragma unroll
        for (int h = 4; h >= 1; h >>= 1) {
#pragma unroll
            for (int i = 0; i < h; ++i) {
                v[i].x += v[i + h].x; v[i].y += v[i + h].y;
                v[i].z += v[i + h].z; v[i].w += v[i + h].w;
            }
        }
        s4.x += v[0].x; s4.y += v[0].y; s4.z += v[0].z; s4.w += v[0].w;
    }
    // 3. fold the row subsets (lane bits 4, 5): lane k ends with the logit of value lane_value(k)
    const float t0 = swap_add32(s4.x, s4.z);
    const float t1 = swap_add32(s4.y, s4.w);
    const float logit = swap_add16(t0, t1);
    const int val = lane_value<ROWS>(lane);
    float resid;
    if constexpr (GRP) {
        // (dp and T are null without DSP, and a link without a dispersion never reads them)
        resid = glm_link<LINK, true>(logit + t.bz + t.ov, t.yv, (int64_t)(val >> 3) < rows_left, ell,
                                     has_v ? t.vv : 1.0f, dp, T);
        // row row0 + (val >> 3) of block row0 >> 4, draw val & 7; nothing lands from the block r_blocks on
        const int64_t blk = row0 >> 4;
        auto rs = bsc_vec_rsrc(ga->R, ga->r_blocks * R_BLOCK, blk * R_BLOCK);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(resid), rs,
                                              4 * ((val & 7) * 16 + (int)(row0 & 8) + (val >> 3)), 0, 0);
    } else if constexpr (ITV)
        resid = glm_link<LINK, true, true>(logit + t.ov, t.yv, (int64_t)(val >> 3) < rows_left, ell,
                                           has_v ? t.vv : 1.0f, dp, T, t.uv);
    else if constexpr (DSP)
        resid = glm_link<LINK, true>(logit + t.ov, t.yv, (int64_t)(val >> 3) < rows_left, ell, has_v ? t.vv : 1.0f,
                                     dp, T);
    else if constexpr (OBS)
        resid = glm_link<LINK, true>(logit + t.ov, t.yv, (int64_t)(val >> 3) < rows_left, ell, has_v ? t.vv : 1.0f);
    else
        resid = glm_link<LINK>(logit, t.yv, (int64_t)(val >> 3) < rows_left, ell);
    float* rb = wl + BSC_WAVE * G8::PSTR;
    rb[val] = resid;
    wave_lds_sync();
    // 4. backward: acc[s] += resid(r, s) * x[r]; residuals arrive by LDS broadcast
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (r == 4) asm volatile("" ::: "memory");  // at most four rows of broadcast reads in flight
        const float4 c0 = *reinterpret_cast<const float4*>(rb + r * SG);
        const float4 c1 = *reinterpret_cast<const float4*>(rb + r * SG + 4);
        axpy4(acc[0], c0.x, t.x[r]); axpy4(acc[1], c0.y, t.x[r]);
        axpy4(acc[2], c0.z, t.x[r]); axpy4(acc[3], c0.w, t.x[r]);
        axpy4(acc[4], c1.x, t.x[r]); axpy4(acc[5], c1.y, t.x[r]);
        axpy4(acc[6], c1.z, t.x[r]); axpy4(acc[7], c1.w, t.x[r]);
    }
}

// The block partial: fixed order over the waves, written in slab order [d][s] | ell[s] (| T[s] at NB_SLAB_STRIDE).
template <int STRIDE = SLAB_STRIDE>
__device__ __forceinline__ void write_block_partial(const float* lds, float* __restrict__ slab, int tid) {
    float* out = slab + (int64_t)blockIdx.x * STRIDE;
    for (int i = tid; i < STRIDE; i += PASS_BLOCK) {
        const int src = i < SLAB_G ? (i & 7) * GCOLS + (i >> 3) : i;
        float v = lds[src];
#pragma unroll
        for (int k = 1; k < PASS_WAVES; ++k) v += lds[k * STRIDE + src];
        out[i] = v;
    }
}

// FULL: D == 256.  n_iter: tiles per wave (the same for every wave; tiles past the end read zeros).
// o, v_: the offset and the weight, each may be null; read only where OBS.
// DSP: logphi [S] (this launch's chunk of the dispersion draws); the slab is NB_SLAB_STRIDE floats per block.
// ITV (with DSP and LINK = GLM_WEIBULL): `upper` [B], not null, rides in the tiles next to y.
template <int LINK, bool FULL, bool OBS, bool GRP = false, bool DSP = false, bool ITV = false>
__device__ __forceinline__ void glm_pass_body(const float* X, int64_t ldx, const float* y, const float* o,
                                              const float* v_, int64_t B, int D, const float* W, int S, float* slab,
                                              int n_iter, const GlmGroupArgs* ga = nullptr,
                                              const float* logphi = nullptr, const float* upper = nullptr) {
    static_assert(!DSP || (OBS && (LINK == GLM_NEGBIN || LINK == GLM_GAMMA || LINK == GLM_WEIBULL || LINK == GLM_BETA)),
                  "the dispersion (the shape) rides with OBS and its own link");
    static_assert(!ITV || (DSP && !GRP && LINK == GLM_WEIBULL),
                  "the upper end rides with the Weibull shape, without groups");
    constexpr int STRIDE = DSP ? NB_SLAB_STRIDE : SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (G8::WAVE_LDS > STRIDE ? G8::WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* wl = lds + wave * G8::WAVE_LDS;
    const bool has_v = OBS && v_ != nullptr;
    GlmDisp dp;
    float tacc = 0.f;
    if constexpr (DSP) dp = glm_disp_of<LINK>(logphi, lane_value<ROWS>(lane) & 7, S);   // before anything fills the file

    float4 w[SG], acc[SG];
#pragma unroll
    for (int s = 0; s < SG; ++s) {
        w[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * lane < D && s < S) w[s] = *reinterpret_cast<const float4*>(W + (int64_t)s * D + 4 * lane);
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float ell = 0.f;

    // This wave owns tiles first, first + stride, ...; every prefetch is unconditional.
    const int64_t stride = (int64_t)gridDim.x * PASS_WAVES;
    int64_t tile = (int64_t)blockIdx.x * PASS_WAVES + wave;
    if constexpr (GRP) {
        // the same rotation; every tile's gather goes out before the loads of the tile after it
        const int* g_ = ga->g;
        const GlmDisp* dq = DSP ? &dp : nullptr;   // (null without DSP, as the defaults of compute_tile are)
        float* tq = DSP ? &tacc : nullptr;
        GlmTile<OBS, GRP> ta, tb;
        load_tile<FULL, OBS, GRP>(ta, X, ldx, y, o, v_, tile * ROWS, B, D, lane, g_);
        for (int k = 0; k + 1 < n_iter; k += 2) {
            gather_tile(ta, *ga, lane);
            load_tile<FULL, OBS, GRP>(tb, X, ldx, y, o, v_, (tile + stride) * ROWS, B, D, lane, g_);
            compute_tile<LINK, OBS, GRP, DSP>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, ga, tile * ROWS, dq,
                                              tq);
            gather_tile(tb, *ga, lane);
            load_tile<FULL, OBS, GRP>(ta, X, ldx, y, o, v_, (tile + 2 * stride) * ROWS, B, D, lane, g_);
            compute_tile<LINK, OBS, GRP, DSP>(tb, w, acc, ell, wl, lane, B - (tile + stride) * ROWS, has_v, ga,
                                              (tile + stride) * ROWS, dq, tq);
            tile += 2 * stride;
        }
        if (n_iter & 1) {
            gather_tile(ta, *ga, lane);
            compute_tile<LINK, OBS, GRP, DSP>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, ga, tile * ROWS, dq,
                                              tq);
        }
    } else {   // (dp and tacc: untouched without DSP)
        GlmTile<OBS, false, ITV> ta, tb;
        load_tile<FULL, OBS>(ta, X, ldx, y, o, v_, tile * ROWS, B, D, lane, nullptr, upper);
        for (int k = 0; k + 1 < n_iter; k += 2) {
            load_tile<FULL, OBS>(tb, X, ldx, y, o, v_, (tile + stride) * ROWS, B, D, lane, nullptr, upper);
            compute_tile<LINK, OBS, false, DSP>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, nullptr, 0, &dp,
                                                &tacc);
            load_tile<FULL, OBS>(ta, X, ldx, y, o, v_, (tile + 2 * stride) * ROWS, B, D, lane, nullptr, upper);
            compute_tile<LINK, OBS, false, DSP>(tb, w, acc, ell, wl, lane, B - (tile + stride) * ROWS, has_v, nullptr,
                                                0, &dp, &tacc);
            tile += 2 * stride;
        }
        if (n_iter & 1)
            compute_tile<LINK, OBS, false, DSP>(ta, w, acc, ell, wl, lane, B - tile * ROWS, has_v, nullptr, 0, &dp,
                                                &tacc);
    }

    __syncthreads();  // every wave is done with its private region
    float* ep = lds + wave * STRIDE;
#pragma unroll
    for (int s = 0; s < SG; ++s) *reinterpret_cast<float4*>(ep + s * GCOLS + 4 * lane) = acc[s];
    // ell of lane k belongs to draw lane_value(k) & 7; fold the tile rows (lane bits 1 .. 3)
    float ev = ell;
    ev += __shfl_xor(ev, 2);
    ev += __shfl_xor(ev, 4);
    ev += __shfl_xor(ev, 8);
    if ((lane & 14) == 0) ep[SLAB_G + (lane_value<ROWS>(lane) & 7)] = ev;
    if constexpr (DSP) {   // T folds like ell
        float tv = tacc;
        tv += __shfl_xor(tv, 2);
        tv += __shfl_xor(tv, 4);
        tv += __shfl_xor(tv, 8);
        if ((lane & 14) == 0) ep[SLAB_G + SG + (lane_value<ROWS>(lane) & 7)] = tv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- 16-row tiles, both contractions on the MFMA pipe (D == 256, y [o, v] 16-byte aligned) ----------------------
constexpr int MT_ROWS = 16;
constexpr int MT_RS = GCOLS + 4;                                // LDS row stride (floats)
constexpr int MT_WAVE_LDS = MT_ROWS * MT_RS + MT_ROWS * SG;     // tile + residuals [draw][row]

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

struct MTileXY {
    float4 x[MT_ROWS];
    float4 yv;     // y[row0 + 4 kq .. + 3]: the rows of this lane's forward result registers
};
template <bool OBS, bool GRP = false, bool ITV = false>
struct MTile : MTileXY {};
template <>
struct MTile<true, false, false> : MTileXY {
    float4 ov, vv;   // offset and weight of the same four rows
};
template <>
struct MTile<true, false, true> : MTileXY {
    float4 ov, vv;
    float4 uv;       // ITV: the upper ends of the same four rows
};
template <>
struct MTile<true, true, false> : MTileXY {
    float4 ov, vv;
    int4 gv;         // group ids of the same four rows
};

__device__ __forceinline__ float4 load_rows4(const float* __restrict__ p, int64_t n, int64_t row0, int lane) {
    auto rs = bsc_vec_rsrc(p, n, row0);
    auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * (lane >> 4), 0, 0);
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

template <bool OBS, bool GRP = false, bool ITV = false>
__device__ __forceinline__ void load_mtile(MTile<OBS, GRP, ITV>& t, const float* __restrict__ X, int64_t ldx,
                                           const float* __restrict__ y, const float* __restrict__ o,
                                           const float* __restrict__ v_, int64_t row0, int64_t B, int lane,
                                           const int* __restrict__ g_ = nullptr,
                                           const float* __restrict__ u_ = nullptr) {
    auto xs = bsc_rows_rsrc(X, ldx, GCOLS, B, row0);
    auto ys = bsc_vec_rsrc(y, B, row0);
    const int lane_off = 16 * lane;
    const int row_bytes = (int)(ldx * 4);
#pragma unroll
    for (int r = 0; r < MT_ROWS; ++r) {
        auto v = __builtin_amdgcn_raw_buffer_load_b128(xs, lane_off, r * row_bytes, 2);   // non-temporal
        t.x[r] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                             __uint_as_float(v[3]));
    }
    auto v = __builtin_amdgcn_raw_buffer_load_b128(ys, 16 * (lane >> 4), 0, 0);
    t.yv = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    if constexpr (OBS) {   // a null vector: no records, every lane reads 0
        t.ov = load_rows4(o, o ? B : 0, row0, lane);
        t.vv = load_rows4(v_, v_ ? B : 0, row0, lane);
    }
    if constexpr (GRP) {
        auto gs = bsc_vec_rsrc(g_, B, row0);
        auto gi = __builtin_amdgcn_raw_buffer_load_b128(gs, 16 * (lane >> 4), 0, 0);
        t.gv = make_int4((int)gi[0], (int)gi[1], (int)gi[2], (int)gi[3]);
    }
    if constexpr (ITV) t.uv = load_rows4(u_, B, row0, lane);
}

template <int LINK, bool OBS, bool GRP = false, bool DSP = false, bool ITV = false>
__device__ __forceinline__ void glm_pass_mfma_body(const float* X, int64_t ldx, const float* y, const float* o,
                                                   const float* v_, int64_t B, const float* W, int S, float* slab,
                                                   int n_iter, const GlmGroupArgs* ga = nullptr,
                                                   const float* logphi = nullptr, const float* upper = nullptr) {
    static_assert(!DSP || (OBS && (LINK == GLM_NEGBIN || LINK == GLM_GAMMA || LINK == GLM_WEIBULL || LINK == GLM_BETA)),
                  "the dispersion (the shape) rides with OBS and its own link");
    static_assert(!ITV || (DSP && !GRP && LINK == GLM_WEIBULL),
                  "the upper end rides with the Weibull shape, without groups");
    constexpr int STRIDE = DSP ? NB_SLAB_STRIDE : SLAB_STRIDE;
    constexpr int LDS_FLOATS = PASS_WAVES * (MT_WAVE_LDS > STRIDE ? MT_WAVE_LDS : STRIDE);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kq = lane >> 4;
    float* tl = lds + wave * MT_WAVE_LDS;      // this wave's tile
    float* rb = tl + MT_ROWS * MT_RS;          // residuals [draw][row]
    const bool has_v = OBS && v_ != nullptr;
    GlmDisp dp;
    float tacc = 0.f;
    if constexpr (DSP) dp = glm_disp_of<LINK>(logphi, i16, S);   // lane (i16, kq) owns draw i16 (live lanes: i16 < 8)

    // forward B operand: W[draw i16][64 kq + 4 j + c]; MFMA columns 8 .. 15 and draws >= S are zero.  Lane group
    // kq contracts columns 64 kq .. 64 kq + 63, which keeps the 16-byte A reads of a lane group conflict-free.
    float wreg[GCOLS / 4];
#pragma unroll
    for (int j = 0; j < GCOLS / 16; ++j) {
        float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i16 < S) w4 = *reinterpret_cast<const float4*>(W + (int64_t)i16 * GCOLS + 64 * kq + 4 * j);
        wreg[4 * j + 0] = w4.x; wreg[4 * j + 1] = w4.y;
        wreg[4 * j + 2] = w4.z; wreg[4 * j + 3] = w4.w;
    }
    mfma_f32x4 acc[2][4];                      // [draw group][column component]: register i = draw 4 sb + i
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[sb][q] = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    float ell = 0.f;
    const bool live = i16 < SG;                // lanes whose forward MFMA column is a draw

    // iteration p of every wave reads one contiguous window of gridDim.x * 4 tiles; p == n_iter: the empty tile
    const int64_t stride0 = (int64_t)gridDim.x * PASS_WAVES;
    const int64_t slot = (int64_t)blockIdx.x * PASS_WAVES + wave;
    auto row0_of = [=](int p) { return p < n_iter ? ((int64_t)p * stride0 + slot) * MT_ROWS : B; };

    const int* g_ = nullptr;
    if constexpr (GRP) g_ = ga->g;
    MTile<OBS, GRP, ITV> t;
    load_mtile<OBS, GRP>(t, X, ldx, y, o, v_, row0_of(0), B, lane, g_, upper);
    for (int p = 0; p < n_iter; ++p) {
        // the tile to LDS, its registers take the next window's tile
#pragma unroll
        for (int r = 0; r < MT_ROWS; ++r) *reinterpret_cast<float4*>(tl + r * MT_RS + 4 * lane) = t.x[r];
        const float4 yv = t.yv;
        float4 ov = make_float4(0.f, 0.f, 0.f, 0.f), vv = make_float4(1.f, 1.f, 1.f, 1.f);
        if constexpr (OBS) {   // this tile's offsets and weights, before the prefetch takes the registers
            ov = t.ov;
            if (has_v) vv = t.vv;
        }
        [[maybe_unused]] float4 uv = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (ITV) uv = t.uv;
        const int64_t rows_left = B - row0_of(p) - 4 * kq;     // rows 4 kq + reg < rows_left are real
        float4 bz = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (GRP) {   // the intercepts of this lane's four rows, ahead of the prefetch and of the forward
            auto bs = glm_bz_rsrc(*ga);
            const int so = 4 * (i16 & 7);
            bz.x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.x + so, 0, 0));
            bz.y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.y + so, 0, 0));
            bz.z = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.z + so, 0, 0));
            bz.w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(bs, 32 * t.gv.w + so, 0, 0));
        }
        load_mtile<OBS, GRP>(t, X, ldx, y, o, v_, row0_of(p + 1), B, lane, g_, upper);
        wave_lds_sync();

        // forward on v_mfma_f32_16x16x4_f32 (two accumulators: no MFMA waits on its predecessor)
        mfma_f32x4 d0 = {0.f, 0.f, 0.f, 0.f}, d1 = {0.f, 0.f, 0.f, 0.f};
        const float* arow = tl + i16 * MT_RS + 64 * kq;
#pragma unroll
        for (int j = 0; j < GCOLS / 16; j += 2) {
            const float4 a0 = *reinterpret_cast<const float4*>(arow + 4 * j);
            const float4 a1 = *reinterpret_cast<const float4*>(arow + 4 * j + 4);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, wreg[4 * j + 0], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, wreg[4 * j + 4], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, wreg[4 * j + 1], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, wreg[4 * j + 5], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, wreg[4 * j + 2], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, wreg[4 * j + 6], d1, 0, 0, 0);
            d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, wreg[4 * j + 3], d0, 0, 0, 0);
            d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, wreg[4 * j + 7], d1, 0, 0, 0);
        }
        // register reg of lane (i16, kq) = logit(row 4 kq + reg, draw i16): the link in the lane, the residuals
        // to rb[draw][row] as one 16-byte store per live lane
        if (live) {
            float r0, r1, r2, r3;
            if constexpr (GRP) {
                const GlmDisp* dq = DSP ? &dp : nullptr;   // (null without DSP, as the defaults of glm_link are)
                float* tq = DSP ? &tacc : nullptr;
                r0 = glm_link<LINK, true>(d0[0] + d1[0] + bz.x + ov.x, yv.x, rows_left > 0, ell, vv.x, dq, tq);
                r1 = glm_link<LINK, true>(d0[1] + d1[1] + bz.y + ov.y, yv.y, rows_left > 1, ell, vv.y, dq, tq);
                r2 = glm_link<LINK, true>(d0[2] + d1[2] + bz.z + ov.z, yv.z, rows_left > 2, ell, vv.z, dq, tq);
                r3 = glm_link<LINK, true>(d0[3] + d1[3] + bz.w + ov.w, yv.w, rows_left > 3, ell, vv.w, dq, tq);
                // block row0 / 16 of R, [draw][row]: nothing lands from the block r_blocks on
                const int64_t blk = row0_of(p) >> 4;
                auto rs = bsc_vec_rsrc(ga->R, ga->r_blocks * R_BLOCK, blk * R_BLOCK);
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                __builtin_amdgcn_raw_buffer_store_b128(
                    u32x4{__float_as_uint(r0), __float_as_uint(r1), __float_as_uint(r2), __float_as_uint(r3)}, rs,
                    4 * (i16 * MT_ROWS + 4 * kq), 0, 0);
            } else if constexpr (ITV) {
                r0 = glm_link<LINK, true, true>(d0[0] + d1[0] + ov.x, yv.x, rows_left > 0, ell, vv.x, &dp, &tacc, uv.x);
                r1 = glm_link<LINK, true, true>(d0[1] + d1[1] + ov.y, yv.y, rows_left > 1, ell, vv.y, &dp, &tacc, uv.y);
                r2 = glm_link<LINK, true, true>(d0[2] + d1[2] + ov.z, yv.z, rows_left > 2, ell, vv.z, &dp, &tacc, uv.z);
                r3 = glm_link<LINK, true, true>(d0[3] + d1[3] + ov.w, yv.w, rows_left > 3, ell, vv.w, &dp, &tacc, uv.w);
            } else if constexpr (DSP) {
                r0 = glm_link<LINK, true>(d0[0] + d1[0] + ov.x, yv.x, rows_left > 0, ell, vv.x, &dp, &tacc);
                r1 = glm_link<LINK, true>(d0[1] + d1[1] + ov.y, yv.y, rows_left > 1, ell, vv.y, &dp, &tacc);
                r2 = glm_link<LINK, true>(d0[2] + d1[2] + ov.z, yv.z, rows_left > 2, ell, vv.z, &dp, &tacc);
                r3 = glm_link<LINK, true>(d0[3] + d1[3] + ov.w, yv.w, rows_left > 3, ell, vv.w, &dp, &tacc);
            } else if constexpr (OBS) {
                r0 = glm_link<LINK, true>(d0[0] + d1[0] + ov.x, yv.x, rows_left > 0, ell, vv.x);
                r1 = glm_link<LINK, true>(d0[1] + d1[1] + ov.y, yv.y, rows_left > 1, ell, vv.y);
                r2 = glm_link<LINK, true>(d0[2] + d1[2] + ov.z, yv.z, rows_left > 2, ell, vv.z);
                r3 = glm_link<LINK, true>(d0[3] + d1[3] + ov.w, yv.w, rows_left > 3, ell, vv.w);
            } else {
                r0 = glm_link<LINK>(d0[0] + d1[0], yv.x, rows_left > 0, ell);
                r1 = glm_link<LINK>(d0[1] + d1[1], yv.y, rows_left > 1, ell);
                r2 = glm_link<LINK>(d0[2] + d1[2], yv.z, rows_left > 2, ell);
                r3 = glm_link<LINK>(d0[3] + d1[3], yv.w, rows_left > 3, ell);
            }
            *reinterpret_cast<float4*>(rb + i16 * MT_ROWS + 4 * kq) = make_float4(r0, r1, r2, r3);
        }
        wave_lds_sync();

        // backward on v_mfma_f32_4x4x1_16B_f32: per row two draw groups x four column components
#pragma unroll
        for (int g = 0; g < MT_ROWS / 4; ++g) {
            if (g) asm volatile("" ::: "memory");   // four rows of reads in flight
            float4 ra[2];
#pragma unroll
            for (int sb = 0; sb < 2; ++sb)
                ra[sb] = *reinterpret_cast<const float4*>(rb + (4 * sb + (lane & 3)) * MT_ROWS + 4 * g);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const float4 x4 = *reinterpret_cast<const float4*>(tl + (4 * g + rr) * MT_RS + 4 * lane);
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) {
                    const float a = rr == 0 ? ra[sb].x : rr == 1 ? ra[sb].y : rr == 2 ? ra[sb].z : ra[sb].w;
                    acc[sb][0] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.x, acc[sb][0], 0, 0, 0);
                    acc[sb][1] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.y, acc[sb][1], 0, 0, 0);
                    acc[sb][2] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.z, acc[sb][2], 0, 0, 0);
                    acc[sb][3] = __builtin_amdgcn_mfma_f32_4x4x1f32(a, x4.w, acc[sb][3], 0, 0, 0);
                }
            }
        }
        wave_lds_sync();   // the next iteration overwrites the tile
    }

    __syncthreads();
    float* ep = lds + wave * STRIDE;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<float4*>(ep + (4 * sb + i) * GCOLS + 4 * lane) =
                make_float4(acc[sb][0][i], acc[sb][1][i], acc[sb][2][i], acc[sb][3][i]);
    float ev = live ? ell : 0.f;               // lane (i16, kq): rows 4 kq .. of draw i16
    ev += __shfl_xor(ev, 16);
    ev += __shfl_xor(ev, 32);
    if (lane < SG) ep[SLAB_G + lane] = ev;
    if constexpr (DSP) {
        float tv = live ? tacc : 0.f;
        tv += __shfl_xor(tv, 16);
        tv += __shfl_xor(tv, 32);
        if (lane < SG) ep[SLAB_G + SG + lane] = tv;
    }
    __syncthreads();
    write_block_partial<STRIDE>(lds, slab, tid);
}

// ---- host side ---------------------------------------------------------------------------------------------------

inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// 16 = the MFMA kernel (needs the full 256-column layout and 16-byte aligned y, offset, weight, group ids and upper
// ends -- null ones count as aligned), else 8-row tiles.
inline int pass_rows(int D, const float* y, const float* o = nullptr, const float* v = nullptr,
                     const int32_t* g = nullptr, const float* u = nullptr) {
    return (D == GCOLS && aligned16(y) && aligned16(o) && aligned16(v) && aligned16(g) && aligned16(u)) ? MT_ROWS
                                                                                                         : ROWS;
}

// The envelope of the entry points that take an offset and a weight: y by name, the vectors' alignment.
inline int check_glm_obs_args(const char* who, int32_t link, const float* X, int64_t ldx, const float* y, const float* o,
                              const float* v, int64_t B, int32_t D, const float* W, int32_t S, int max_s) {
    BSC_REQUIRE(link == BSC_GLM_LOGISTIC || link == BSC_GLM_POISSON,
                "%s: link=%d must be BSC_GLM_LOGISTIC (0) or BSC_GLM_POISSON (1)", who, link);
    BSC_REQUIRE(y || B <= 0, "%s: y is null with B=%lld", who, (long long)B);
    BSC_REQUIRE((((uintptr_t)o) & 3) == 0 && (((uintptr_t)v) & 3) == 0, "%s: offset and weight must be 4-byte aligned",
                who);
    return check_regress_args(who, X, ldx, B, D, W, S, max_s);
}

// The three kernels of a route: 16-row MFMA tiles, else 8-row tiles with D == 256 (FULL) or any D.  rows8 takes FULL
// as std::true_type / std::false_type, so that the launch site names its 8-row kernel once.
template <class Mfma, class Rows8>
void launch_pass_shape(int rows, int D, Mfma mfma, Rows8 rows8) {
    if (rows == MT_ROWS) mfma();
    else if (D == GCOLS) rows8(std::true_type{});
    else rows8(std::false_type{});
}

// All S draws, eight per launch: pass(s0, sg) launches the pass over draws s0 .. s0 + sg - 1 (timed alone),
// reduce(s0) its slab reduction; tail(s0) is what else the chunk needs (the group sums) and returns a status.
template <class Pass, class Reduce, class Tail>
int for_draw_chunks(bsc_ctx* ctx, int S, Pass pass, Reduce reduce, Tail tail) {
    for (int s0 = 0; s0 < S; s0 += SG) {
        const int sg = S - s0 < SG ? S - s0 : SG;
        {
            bsc_prof_scope prof(ctx);  // times the pass kernel alone
            pass(s0, sg);
        }
        BSC_LAUNCH_CHECK();
        reduce(s0);
        BSC_LAUNCH_CHECK();
        const int rc = tail(s0);
        if (rc != BSC_OK) return rc;
    }
    return BSC_OK;
}

template <class Pass, class Reduce>
int for_draw_chunks(bsc_ctx* ctx, int S, Pass pass, Reduce reduce) {
    return for_draw_chunks(ctx, S, pass, reduce, [](int) { return (int)BSC_OK; });
}

// (The data pass of the DSP routes, kernels and host side: csrc/bsc_scalar_family.h.)

}  // namespace

// The launch of the OBS kernels, defined in csrc/bsc_glm_obs.hip and called from csrc/bsc_glm.hip:

// 16-row MFMA tiles when mfma != 0 (D == 256; y and the set ones of o, v 16-byte aligned), else 8-row VALU tiles.
void bsc_glm_obs_launch_pass(bsc_ctx* ctx, int link, int mfma, const float* X, int64_t ldx, const float* y,
                             const float* offset, const float* weight, int64_t B, int D, const float* W, int sg,
                             int n_blocks, int n_iter, float* slab);
