// Everything a likelihood family is, one struct per family: its ids, whether a learned log-scalar rides with every draw,
// the per-launch constants of a draw and the link, for the training pass (csrc/bsc_glm_pass.h) and for the predictive
// pass (csrc/bsc_predict_pass.h).  The passes take a family as a type and know none by name; GlmFamily<LINK> and
// PredictFamily<FAM> at the end map the integer ids, which the __global__ kernel templates keep as their parameters, to
// the structs.  A new family with a learned scalar is a struct here, its ids, and three extern "C" functions
// (csrc/bsc_scalar_family.h).  Header-only, internal linkage, like csrc/bsc_regress.h.
//
// A struct holds, where its family has the side:
//   GLM_ID, PREDICT_ID, SCALAR_ID   the internal ids (public where a BSC_* constant of include/bayesic_hip.h spells them)
//   SCALAR        a per-draw log-scalar tau_s rides behind the weights (training: the slab gets T[s] = d ell[s] / d tau_s)
//   glm_disp      training: what a lane keeps of its draw's scalar, made once per launch
//   glm_link      training: ell += v (log p) for a real row, T likewise, returns resid = d / d l
//   PER_DRAW, predict_slots   prediction: the per-draw constants, [slot][P_MAX_S] floats in the LDS
//   predict_link  prediction: mu, v and log p(y | l) of one (row, draw): (l, y, the row's `upper` entry, slots 0 .. 2,
//                 outputs, slot 3)
//   ROW_LGAMMA    prediction: lnGamma(y + 1) is taken off once per row, after the log-mean-exp
//   PARAM         a constant of the model (the Student-t's degrees of freedom) rides with the launch as one float: glm_disp
//                 and predict_slots take it as a last argument, and the kernels are the scalar_par_* ones
//                 (csrc/bsc_scalar_family.h), which have it as theirs
//
// The kernels are compared instruction by instruction when a family moves (profiles/family_refactor_isa.txt).  What
// keeps them as they are: a link is ONE function (the compiler simplifies every function on its own before it inlines
// it: a helper around half a link orders its selects differently); it takes the row's fields as scalars by value, the
// draw's scalar and T as plain pointers (a reference may be read ahead of a select); and its arguments are made in the
// caller in the order of its parameters.
#pragma once

#include "bsc_regress.h"
#include "bsc_special_f32.h"

namespace {

constexpr int P_MAX_S = 64;                    // draws of a predictive launch at most: the stride of the slots
// The cumulative-logit family keeps its own branch of predict_body and its own training unit (csrc/bsc_glm_ordinal.hip:
// predict_ordinal_kernel, bsc_ordinal_predict_pass), K - 1 cutpoints per draw.  Always with OFFS, the offset may be null;
// y holds the bits of int32 labels; the outputs are prob [B, K] (PredictOrdinal) and lpd, no mean and no var.
constexpr int PREDICT_ORDINAL = 6;

// What a lane keeps of its draw's scalar in training: tau_s as the pass read it, e^tau, and two constants of the family's.
struct GlmDisp {
    float tau, phi;
    float lg, psi;
};

// Draw s of this launch's chunk (s >= S: a dead slot, phi = 1).
__device__ __forceinline__ GlmDisp glm_disp_tau(const float* logphi, int s, int S) {
    GlmDisp d;
    d.tau = s < S ? logphi[s] : 0.0f;
    d.phi = expf(d.tau);
    return d;
}

// One row as a pass hands it to a training link (glm_link at the end).  v and u are set only where the pass carries them
// (OBS, ITV).
struct GlmRow {
    float y;
    float v = 1.0f;     // the weight; a link scales both terms by it where v > 0 and adds exactly 0 elsewhere
    float u = 0.0f;     // ITV: the row's entry of `upper` (Weibull::glm_link_upper says how it is read)
    bool real;          // the row is inside the batch
};

// Slots 0 .. 2 of draw s (gp[k * P_MAX_S + s] is slot k): logvar, exp(logvar), exp(-logvar).
__device__ __forceinline__ void predict_slots3(float* gp, int s, float lv) {
    gp[s] = lv;
    gp[P_MAX_S + s] = expf(lv);
    gp[2 * P_MAX_S + s] = expf(-lv);
}

// What the families without a learned scalar share.  In their links, OBS: `l` already holds the offset; both terms are
// scaled by the weight vv where vv > 0 and are exactly 0 elsewhere.
struct PlainFamily {
    static constexpr int GLM_ID = -1;              // no training pass of csrc/bsc_glm_pass.h
    static constexpr bool SCALAR = false, PER_DRAW = false, ROW_LGAMMA = false, UPPER = false;
    static constexpr bool PARAM = false;           // no per-model constant rides with the launch
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) { predict_slots3(gp, s, lv); }
};

// ---- logistic: ell += y l - A(l), resid = y - A'(l) --------------------------------------------------------------------
// A = softplus in the stable form max(l, 0) + log1p(e), e = exp(-|l|) <= 1 (exp at full float32 accuracy: the tails at
// |l| = 80 are compared at rtol 1e-6), and A' = sigmoid from the same e (1 / (1 + e) for l >= 0, e / (1 + e) below): finite
// for every finite l.
// Prediction: mu = sigmoid, v = mu (1 - mu) = e / (1 + e)^2 without the cancellation, softplus with log1p(e) =
// log(t) e / (t - 1), t = 1 + e (the quotient undoes the rounding of t): finite for every finite l.
struct Logistic : PlainFamily {
    static constexpr int GLM_ID = BSC_GLM_LOGISTIC, PREDICT_ID = BSC_PREDICT_LOGISTIC;
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp*, float*, float) {
        const float e = expf(-fabsf(l));
        const float t = 1.0f + e;
        const float rc = __builtin_amdgcn_rcpf(t);
        const float da = l >= 0.0f ? rc : e * rc;
        // log1p(e) = log(t) e / (t - 1): the quotient undoes the rounding of t = 1 + e (t - 1 is exact); t == 1: e itself.
        // Within 3e-7 of log1p over e in [0, 1], ten vector instructions where the library's log1pf is ~90.
        const float lp = t == 1.0f ? e : __logf(t) * e * __builtin_amdgcn_rcpf(t - 1.0f);
        const float a = fmaxf(l, 0.0f) + lp;
        if (OBS) {
            const bool on = vv > 0.0f;
            ell += (real_row && on) ? vv * fmaf(yv, l, -a) : 0.0f;
            return on ? vv * (yv - da) : 0.0f;
        }
        ell += real_row ? fmaf(yv, l, -a) : 0.0f;
        return yv - da;
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        const float e = expf(-fabsf(l));
        const float t = 1.0f + e;
        const float r = 1.0f / t;
        mu = l >= 0.0f ? r : e * r;
        v = e * r * r;
        const float l1p = t == 1.0f ? e : logf(t) * e / (t - 1.0f);
        lp = fmaf(yv, l, -(fmaxf(l, 0.0f) + l1p));
    }
};

// ---- Poisson: A = A' = exp(l), NOT clamped (a clamp would change the gradient silently): finite for l <= 88 -----------
// Prediction: mu = v = exp(l); the row constant lnGamma(y + 1) is taken off after the log-mean-exp.
struct Poisson : PlainFamily {
    static constexpr int GLM_ID = BSC_GLM_POISSON, PREDICT_ID = BSC_PREDICT_POISSON;
    static constexpr bool ROW_LGAMMA = true;
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp*, float*, float) {
        const float a = expf(l), da = a;
        if (OBS) {
            const bool on = vv > 0.0f;
            ell += (real_row && on) ? vv * fmaf(yv, l, -a) : 0.0f;
            return on ? vv * (yv - da) : 0.0f;
        }
        ell += real_row ? fmaf(yv, l, -a) : 0.0f;
        return yv - da;
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        mu = expf(l);
        v = mu;
        lp = fmaf(yv, l, -mu);
    }
};

// ---- Gaussian (predictive only): slots (logvar, exp(logvar), exp(-logvar)), logvar = log s2 per draw -------------------
struct Gaussian : PlainFamily {
    static constexpr int PREDICT_ID = BSC_PREDICT_GAUSSIAN;
    static constexpr bool PER_DRAW = true;
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        const float r = yv - l;
        mu = l;
        v = ev;
        lp = fmaf(-0.5f * iv * r, r, -0.5f * (lv + (float)BSC_LOG_2PI));
    }
};

// The ordinal family's constant and the flags predict_body reads of it; its link is predict_body's own branch.
struct Ordinal : PlainFamily {
    static constexpr int PREDICT_ID = PREDICT_ORDINAL;
};

// What the families with a learned scalar share: always OBS (dp and T set), the offset may be null in prediction, and
// `logvar` carries tau_s.  A lane owns ONE draw in both tile shapes of the pass, so glm_disp's values stay in four
// registers; the special values are made in float64, once per launch, then rounded.
// The selects of every link here sit on the INPUTS: a dropped row (weight 0, or past B) is evaluated at a harmless point
// -- finite whatever it held -- and its terms are multiplied by an exact 0.  A select on the results turns into a branch
// around the whole evaluation, which splits the loop body and spills.  Each select is flat, between values at hand: a
// nested one (keep ? (left ? .. : ..) : ..) comes out as a branch that the logit's last additions sink into, which splits
// the loop body and spills 150 bytes per lane.
struct ScalarFamily {
    static constexpr bool SCALAR = true, PER_DRAW = true, ROW_LGAMMA = false;
    static constexpr bool UPPER = false;           // the links take no upper ends
    static constexpr bool PARAM = false;           // no per-model constant: glm_disp and predict_slots take none
    // (tau, phi = e^tau, lnGamma(phi), psi(phi)): the negative binomial's and the Beta family's
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        d.lg = (float)bsc_lgamma_f64((double)d.phi);
        d.psi = (float)bsc_digamma_f64((double)d.phi);
        return d;
    }
};

// ---- negative binomial: tau = log phi, the dispersion; internal ids (the BSC_GLM_* / BSC_PREDICT_* entry points refuse
// them): csrc/bsc_glm_nb.hip (bsc_nb_predict_pass) ----------------------------------------------------------------------
// glm_disp: (tau, phi, lnGamma(phi), psi(phi)).  With u = l - tau, z = y + phi and the logistic forms at u,
//     ell  += v [ dlnGamma(y, phi) + y u - z softplus(u) ]          dlnGamma = lnGamma(z) - lnGamma(phi)
//     resid = v [ y - z sigmoid(u) ]                                                           (= d / d l)
//     T    += v [ phi dpsi(y, phi) - phi softplus(u) ] - resid       dpsi = psi(z) - psi(phi)   (= d / d tau)
// finite for every finite l; both differences are exactly 0 at y = 0 (csrc/bsc_special_f32.h: an empty product).
// Prediction: slots (tau, phi, 1 / phi, lnGamma(phi)).  mu = exp(l) (not clamped), v = mu + mu^2 / phi; log p from the
// logistic forms at u = l - tau, finite for every finite l: lnGamma(y + phi) - lnGamma(phi) + y u - (y + phi) softplus(u),
// the difference exactly 0 at y = 0; the row constant lnGamma(y + 1) is taken off after the log-mean-exp.
struct NegBin : ScalarFamily {
    static constexpr int GLM_ID = 2, PREDICT_ID = 3, SCALAR_ID = BSC_SCALAR_NEGBIN;
    static constexpr bool ROW_LGAMMA = true;
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at y = 0, u = 0
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.0f;
        const float u = keep ? l - dp->tau : 0.0f;
        const float e = expf(-fabsf(u));
        const float t = 1.0f + e;
        const float rc = __builtin_amdgcn_rcpf(t);
        const float sig = u >= 0.0f ? rc : e * rc;
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
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) {
        predict_slots3(gp, s, lv);
        gp[3 * P_MAX_S + s] = (float)bsc_lgamma_f64((double)expf(lv));
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        mu = expf(l);
        v = fmaf(mu * iv, mu, mu);
        const float u = l - lv;
        const float e = expf(-fabsf(u));
        const float t = 1.0f + e;
        const float l1p = t == 1.0f ? e : logf(t) * e / (t - 1.0f);
        float dlg, dps;
        bsc_dlgamma_dpsi_f32(yv, ev, lgp, 0.0f, dlg, dps);      // (dpsi is not used and folds away)
        lp = dlg + fmaf(yv, u, -(yv + ev) * (fmaxf(u, 0.0f) + l1p));
    }
};

// ---- Gamma: tau = log alpha, the shape; internal ids: csrc/bsc_glm_gamma.hip (bsc_gamma_predict_pass) -------------------
// glm_disp: (tau, alpha, c_a = alpha log alpha - lnGamma(alpha), c_1 = log alpha + 1 - psi(alpha)).  y > 0, ly = log y,
// q = y e^{-l}:
//     ell  += v [ c_a + alpha (ly - l - q) - ly ]                    (the full density, nothing left out)
//     resid = v alpha (q - 1)                                                                  (= d / d l)
//     T    += v alpha (c_1 + ly - l - q)                                                       (= d / d tau)
// NOT clamped, like the Poisson link: finite while e^{-l} and y e^{-l} are below the float32 maximum (l > -88 at
// y = 1).  One exp and one log per (row, draw), both at full float32 accuracy: ly enters ell multiplied by alpha.
// Prediction: slots (tau, alpha, 1 / alpha, c_a).  mu = exp(l) (not clamped), v = mu^2 / alpha; log p = c_a +
// alpha (log y - l - y e^{-l}) - log y, the full density in the training forms (the exponential as the product y e^{-l});
// y > 0 is the caller's to see to.
struct Gamma : ScalarFamily {
    static constexpr int GLM_ID = 3, PREDICT_ID = 4, SCALAR_ID = BSC_SCALAR_GAMMA;
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        const double a = (double)d.phi, la = log(a);
        d.lg = (float)(a * la - bsc_lgamma_f64(a));
        d.psi = (float)(la + 1.0 - bsc_digamma_f64(a));
        return d;
    }
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at y = 1, l = 0 -- every term finite, log 0 never formed
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
    // (slots 0 .. 2 here; slot 3, c_a, is written by predict_body itself, next to this call: made in here, the compiler
    // orders its float64 logarithm and lnGamma the other way round and the kernels change)
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) { predict_slots3(gp, s, lv); }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        mu = expf(l);
        v = mu * iv * mu;
        const float ly = logf(yv);
        lp = fmaf(ev, (ly - l) - yv * expf(-l), lgp) - ly;
    }
};

// ---- Weibull: tau = log k, the shape; internal ids: csrc/bsc_glm_weibull.hip (bsc_weibull_predict_pass) and, with upper
// ends, csrc/bsc_glm_weibull_interval.hip ------------------------------------------------------------------------------
// glm_disp: (tau, k, 0, 0) -- the density has no special function in it.  The sign of y is the censoring flag -- y > 0 an
// event at y, y < 0 right-censored at -y -- so delta = (y > 0), t = |y| and the tiles carry nothing new; ly = log t,
// z = k (ly - l), l the log SCALE:
//     ell  += v [ delta (tau + z - ly) - e^z ]            (log f = tau + z - ly - e^z, log S = -e^z: nothing left out)
//     resid = v k (e^z - delta)                                                                (= d / d l)
//     T    += v [ delta (1 + z) - z e^z ]                                                      (= d / d tau)
// NOT clamped, like the Poisson and Gamma links: finite while z stays below about 88 (e^z and z e^z below the float32
// maximum).  One log and one exp per (row, draw) at full float32 accuracy; z is rounded before the exponential, which
// costs |z| eps of e^z (the tests' bounds count (1 + |z|) e^z per row).  y = 0 or a non-finite y on a kept row is the
// caller's to keep out.
// ITV (glm_link_upper): `u` is the row's entry of the vector `upper` -- 0: the row is what y says, as above; u > 0 (with
// y < 0): interval-censored on (a, b] = (-y, u]; u < 0: left-censored at b = -u, the magnitude of y not read.  With
// z = k (log a - l), E = e^z, d = log b - log a and Delta = E expm1(k d) = E_b - E_a (a left-censored row:
// z = k (log b - l), Delta = E, and E_a = 0 in what follows), e = e^{-Delta}, p = -expm1(-Delta):
// (d through log1p((b - a) / a) where b < 2 a: the difference of two rounded logarithms would lose a narrow interval)
//     ell  += v [ -E_a + log p ]                                       (= log(S(a) - S(b)): nothing left out)
//     resid = v k ( E_a - Delta e / p )                                (Delta e / p = Delta / expm1(Delta), in (0, 1))
//     T    += v [ -z E_a + (z Delta + k d E_b) e / p ]                 E_b = E_a + Delta
// all three in ONE form with the rows above: an indicator `ic` (1 on such a row, else 0) multiplies the new terms, which
// a row without an upper end evaluates at Delta = 1, k d = 0.  OVERFLOW: where Delta >= ITV_BIG -- e^{-Delta} is zero in
// float32 (csrc/bsc_special_f32.h), or the upper end is so far out that e^{k d} or Delta is infinite (upper = 1e30 for "no
// bound") -- the row is the right-censored one at a (the left-censored one adds nothing: its probability is 1), by the
// same select on the inputs; a NaN Delta (0 times infinity) goes the same way.  Seven transcendentals per (row, draw) for
// two.
// Prediction: slots (tau, k, g1 = Gamma(1 + 1/k), g2 = Gamma(1 + 2/k) - Gamma(1 + 1/k)^2), both made once per launch in
// float64 (the exp(-logvar) slot is not needed and carries g1).  mu = e^l g1, v = e^{2l} g2 (not clamped); with t = |y|,
// z = k (log t - l):  log p = tau + z - log t - e^z for y > 0 (an event at y), log p = -e^z for y < 0 (right-censored at
// -y: the log survival), so the lpd of a censored row is the log of the posterior-predictive survival probability.  y = 0
// is the caller's to keep out.  ITV (predict_link_upper): `u` is read as glm_link_upper reads it, the same forms and the
// same overflow rule: log p = -E_a + log(-expm1(-Delta)), the log of the row's probability, so its lpd is the log of the
// draw average of that probability.  mu and v do not depend on the row's kind.
// FLOAT32 ENVELOPE OF THE MOMENTS: Gamma(1 + 2/k) overflows float32 near k = 0.06 (tau = -2.8); accuracy envelope tau in
// [-2, 4].  g2 is a difference of float64 values, 5e-4 at tau = 4: no digit of the float32 result is lost to it.
struct Weibull : ScalarFamily {
    static constexpr int GLM_ID = 4, PREDICT_ID = 5, SCALAR_ID = BSC_SCALAR_WEIBULL;
    static constexpr bool UPPER = true;
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        d.lg = d.psi = 0.0f;
        return d;
    }
    static __device__ __forceinline__ float glm_link_upper(float l, float yv, bool real_row, float& ell, float vv,
                                                           const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at a = b = 1, l = 0, delta = 0, ic = 0
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
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        if constexpr (ITV) return glm_link_upper(l, yv, real_row, ell, vv, dp, T, uv);
        // a dropped row is evaluated at t = 1, l = 0, delta = 0 -- z = 0, every term finite whatever y held (0 and NaN
        // included)
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
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) {
        predict_slots3(gp, s, lv);
        const double ik = 1.0 / (double)expf(lv);
        const double g1 = exp(bsc_lgamma_f64(1.0 + ik));
        gp[2 * P_MAX_S + s] = (float)g1;
        gp[3 * P_MAX_S + s] = (float)(exp(bsc_lgamma_f64(1.0 + 2.0 * ik)) - g1 * g1);
    }
    static __device__ __forceinline__ void predict_link_upper(float l, float yv, float uv, float lv, float ev, float iv,
                                                              float& mu, float& v, float& lp, float lgp) {
        const float el = expf(l);
        mu = el * iv;
        v = el * lgp * el;
        const bool left = uv < 0.0f, itv = uv > 0.0f;
        const float tq = fabsf(left ? uv : yv);
        const float bq = itv ? uv : tq;
        const float ly = logf(tq);
        const float z = ev * (ly - l);
        const float ez = expf(z);
        const float kd = ev * bsc_logratio_f32(bq, tq, ly);    // exactly 0 unless the row is an interval
        const float dlt = ez * (bsc_expm1_f32(kd) + (left ? 1.0f : 0.0f));   // expm1(0) = 0 on a left-censored row
        const bool on = (left || itv) && dlt < ITV_BIG;         // false for a NaN as well
        const float dq = on ? dlt : 1.0f;
        const float ea = left ? 0.0f : ez;
        const float lpc = fmaf(on ? 1.0f : 0.0f, logf(-bsc_expm1_f32(-dq)), -ea);
        lp = (uv == 0.0f && yv > 0.0f) ? ((lv + z) - ly) - ez : lpc;
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        if constexpr (ITV) return predict_link_upper(l, yv, uv, lv, ev, iv, mu, v, lp, lgp);
        const float el = expf(l);
        mu = el * iv;
        v = el * lgp * el;
        const float ly = logf(fabsf(yv));
        const float z = ev * (ly - l);
        const float ez = expf(z);
        lp = yv > 0.0f ? ((lv + z) - ly) - ez : -ez;
    }
};

// ---- Beta: tau = log phi, the precision of the mean / precision form; internal ids: csrc/bsc_glm_beta.hip
// (bsc_beta_predict_pass) ---------------------------------------------------------------------------------------------
// glm_disp: the negative binomial's (tau, phi, lnGamma(phi), psi(phi)).  0 < y < 1, ly = log y, l1y = log1p(-y),
// m = sigmoid(l) and 1 - m = sigmoid(-l) EACH from the stable logistic forms e / (1 + e), 1 / (1 + e) with e = exp(-|l|)
// (never 1 - m by subtraction), a = m phi, b = (1 - m) phi:
//     ell  += v [ lnGamma(phi) - lnGamma(a) - lnGamma(b) + (a - 1) ly + (b - 1) l1y ]    (the full density, nothing left out)
//     resid = v phi m (1 - m) [ (ly - l1y) - psi(a) + psi(b) ]                                (= d / d l)
//     T    += v phi [ psi(phi) + m (ly - psi(a)) + (1 - m)(l1y - psi(b)) ]                     (= d / d tau)
// lnGamma and psi of a and of b are float32, per (row, draw), from csrc/bsc_special_f32.h's bsc_lgamma_psi_f32, one
// evaluation after the other: four logs, four reciprocals and two shifted products per (row, draw) on top of the logistic
// link's exp.  l1y through log(w) (-y) / (w - 1), w = 1 - y, which undoes the rounding of w (y = 1e-6: log(1 - y) alone is
// 6 % off).  NOT clamped: finite while a, b and their reciprocals are normal float32 values -- |l| <= 80 at tau in
// [-2, 5], where psi(a) ~ -1 / a reaches 4e35 and is multiplied by m before anything else.  y = 0, y = 1 or a non-finite
// y on a kept row is the caller's to keep out.
// Prediction: slots (tau, phi, 1 / (1 + phi), lnGamma(phi)), both made once per launch in float64 (the exp(-logvar) slot
// carries the variance factor).  mu = m, v = m (1 - m) / (1 + phi) with m (1 - m) = e / (1 + e)^2; log p the full density
// in the training forms (bsc_lgamma_psi_f32 whose psi half folds away); 0 < y < 1 is the caller's to see to.
struct Beta : ScalarFamily {
    static constexpr int GLM_ID = 5, PREDICT_ID = 7;
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at y = 1/2, l = 0 -- a = b = phi / 2, every term finite whatever y and l held
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.5f;
        const float lq = keep ? l : 0.0f;
        const float e = expf(-fabsf(lq));
        const float rc = __builtin_amdgcn_rcpf(1.0f + e);
        const float er = e * rc;
        const bool pos = lq >= 0.0f;
        const float m = pos ? rc : er, m1 = pos ? er : rc;       // sigmoid(l) and sigmoid(-l), neither by subtraction
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
        return vq * ((dp->phi * (er * rc)) * (((ly - l1y) - psa) + psb));
    }
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) {
        predict_slots3(gp, s, lv);
        const double ph = (double)expf(lv);
        gp[2 * P_MAX_S + s] = (float)(1.0 / (1.0 + ph));
        gp[3 * P_MAX_S + s] = (float)bsc_lgamma_f64(ph);
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        const float e = expf(-fabsf(l));
        const float r = __builtin_amdgcn_rcpf(1.0f + e);
        const float er = e * r;
        const bool pos = l >= 0.0f;
        const float m = pos ? r : er, m1 = pos ? er : r;
        mu = m;
        v = er * r * iv;
        const float ly = logf(yv);
        const float w = 1.0f - yv;
        const bool one = w == 1.0f;
        const float l1y = fmaf(logf(w), yv * __builtin_amdgcn_rcpf(one ? 1.0f : 1.0f - w), one ? -yv : 0.0f);
        const float a = m * ev, b = m1 * ev;
        float lga, psa, lgb, psb;                               // (psi is not used and folds away)
        bsc_lgamma_psi_f32(a, lga, psa);
        bsc_lgamma_psi_f32(b, lgb, psb);
        lp = ((lgp - lga) - lgb) + fmaf(a - 1.0f, ly, (b - 1.0f) * l1y);
    }
};

// ---- log-normal: tau = log(1 / sigma), the log of the INVERSE scale; internal ids: csrc/bsc_glm_lognormal.hip
// (bsc_lognormal_predict_pass) ------------------------------------------------------------------------------------------
// glm_disp: (tau, k = 1 / sigma = e^tau, 0, 0) -- the density has no per-draw constant.  The sign of y is the censoring
// flag as in the Weibull family -- y > 0 an event at y, y < 0 right-censored at -y -- so delta = (y > 0), t = |y|,
// ly = log t, z = k (ly - l), l the LOCATION of log t (the Weibull link's z, rounded the same way); with
// (lsf, h) = (log Phi(-z), phi(z) / Phi(-z)) from csrc/bsc_special_f32.h's bsc_lognormsf_hazard_f32:
//     ell  += v [ delta (tau - ly - z^2 / 2 - log(2 pi) / 2) + (1 - delta) lsf ]    (log f and log S: nothing left out)
//     resid = v k [ delta z + (1 - delta) h ]                                                  (= d / d l)
//     T    += v [ delta (1 - z^2) - (1 - delta) z h ]                                          (= d / d tau)
// NOT clamped and no need to be: every term is finite for every finite z whose square is (|z| < 1.8e19), both tails of
// the censored rows included -- the Weibull link's z < 88 does not apply.  One log, one erfcx, one exp, one more log and
// one reciprocal per (row, draw).  y = 0 or a non-finite y on a kept row is the caller's to keep out.
// Prediction: slots (tau, k, m1 = e^{sigma^2 / 2}, m2 = (e^{sigma^2} - 1) e^{sigma^2}), sigma^2 = e^{-2 tau}, both made
// once per launch in float64 from tau itself (the exp(-logvar) slot is not needed and carries m1).  mu = e^l m1,
// v = e^{2l} m2 (not clamped); log p = tau - log t - z^2 / 2 - log(2 pi) / 2 for y > 0 (an event at y), log p = lsf for
// y < 0 (right-censored at -y: the log survival), so the lpd of a censored row is the log of the posterior-predictive
// survival probability.  y = 0 is the caller's to keep out.
// FLOAT32 ENVELOPE OF THE MOMENTS: m2 ~ e^{2 sigma^2} overflows float32 at sigma^2 = 44.4 (tau = -1.90; at tau = -2
// sigma^2 = 54.6); accuracy envelope tau in [-1.5, 4] (sigma from 4.5 down to 0.018, m2 = 2.8e17 at the lower end).  m2
// through expm1 in float64: 3e-4 at tau = 4 with every digit.
struct LogNormal : ScalarFamily {
    static constexpr int GLM_ID = 6, PREDICT_ID = 8;
    static constexpr bool UPPER = false;           // right censoring alone: no upper ends
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        d.lg = d.psi = 0.0f;
        return d;
    }
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at t = 1, l = 0, delta = 0 -- z = 0, every term finite whatever y held (0 and NaN
        // included)
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float tq = keep ? fabsf(yv) : 1.0f;
        const float dl = (keep && yv > 0.0f) ? 1.0f : 0.0f;
        const float lq = keep ? l : 0.0f;
        const float ly = logf(tq);
        const float z = dp->phi * (ly - lq);
        float lsf, hz;
        bsc_lognormsf_hazard_f32(z, lsf, hz);
        const float cs = 1.0f - dl;
        const float zz = z * z;
        ell = fmaf(vq, fmaf(dl, (dp->tau - ly) - fmaf(0.5f, zz, 0.5f * (float)BSC_LOG_2PI), cs * lsf), ell);
        *T = fmaf(vq, fmaf(dl, 1.0f - zz, -cs * (z * hz)), *T);
        return vq * (dp->phi * fmaf(dl, z, cs * hz));
    }
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) {
        predict_slots3(gp, s, lv);
        const double s2 = exp(-2.0 * (double)lv);
        gp[2 * P_MAX_S + s] = (float)exp(0.5 * s2);
        gp[3 * P_MAX_S + s] = (float)(expm1(s2) * exp(s2));
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        const float el = expf(l);
        mu = el * iv;
        v = el * lgp * el;
        const float ly = logf(fabsf(yv));
        const float z = ev * (ly - l);
        float lsf, hz;                                          // (the hazard is not used and folds away)
        bsc_lognormsf_hazard_f32(z, lsf, hz);
        lp = yv > 0.0f ? (lv - ly) - fmaf(0.5f * z, z, 0.5f * (float)BSC_LOG_2PI) : lsf;
    }
};

// ---- zero-inflated Poisson: tau = log omega, the log ODDS of a structural zero, pi = sigmoid(tau); internal ids:
// csrc/bsc_glm_zip.hip (bsc_zip_predict_pass) -----------------------------------------------------------------------------
// glm_disp: (tau, omega = e^tau, L1 = log1p(omega) = softplus(tau), pi = sigmoid(tau)), the last two made once per launch
// in float64 and rounded, in the two slots the negative binomial fills with lnGamma and psi.  y is a count; mu = e^l,
// u = tau + mu, e = e^{-|u|}, and sigmoid(u), sigmoid(-u) EACH from the stable logistic forms 1 / (1 + e), e / (1 + e)
// (never one by subtraction from the other).  The two branches are chosen by y == 0:
//                     y == 0                                             y > 0
//     log p    max(tau, -mu) + log1p(e) - L1                             y l - mu - L1
//     d / d l  -mu r,   r = sigmoid(-u) = P(Poisson | y = 0)             y - mu
//     d / d tau  sigmoid(u) (1 - pi) (-expm1(-mu))                       -pi
//     ell  += v log p,    resid = v d / d l,    T += v d / d tau
// The zero branch is log(omega + e^{-mu}) - log1p(omega), written so that softplus(u) - mu is never formed; its tau
// derivative is sigmoid(u) - sigmoid(tau), which cancels at small mu, as the product of three factors in [0, 1]: never
// negative.  Training leaves the row constant -lnGamma(y + 1) out, as the Poisson and negative-binomial links do.  Both
// branches are evaluated for every row and chosen by flat selects between values at hand (y l = 0 on a zero row, so the
// positive branch is finite there, and the zero branch is finite everywhere).  NOT clamped, like the Poisson link: finite
// while e^l is.  At l = +80 a zero row gives e = 0, so log p = tau - L1 = log pi, d / d l = -mu 0 = 0 and d / d tau =
// 1 - pi, each exactly.  Per (row, draw) on top of the Poisson link's exp: e^{-|u|} with its reciprocal, log1p (a log and
// a division) and expm1 (e^{-mu}, a log and a reciprocal).
// Prediction: slots (tau, omega, pi, L1), pi and L1 made once per launch in float64 (the exp(-logvar) slot carries pi).
// mu = (1 - pi) e^l, v = (1 - pi) e^l (1 + pi e^l) (not clamped); log p in the training forms; the row constant
// lnGamma(y + 1) is taken off after the log-mean-exp (lnGamma(1) = 0 keeps the zero rows right).
struct ZeroInflPoisson : ScalarFamily {
    static constexpr int GLM_ID = 7, PREDICT_ID = 9;
    static constexpr bool ROW_LGAMMA = true;
    static constexpr bool UPPER = false;
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        const double t = (double)d.tau, e = exp(-fabs(t));
        d.lg = (float)(fmax(t, 0.0) + log1p(e));
        d.psi = (float)((t >= 0.0 ? 1.0 : e) / (1.0 + e));
        return d;
    }
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at y = 0, l = 0 -- every term finite whatever y held (NaN and negatives included)
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.0f;
        const float lq = keep ? l : 0.0f;
        const float mu = expf(lq);
        const float u = dp->tau + mu;
        const float e = expf(-fabsf(u));
        const float t = 1.0f + e;
        const float rc = __builtin_amdgcn_rcpf(t);
        const float er = e * rc;
        const bool pos = u >= 0.0f;
        const float su = pos ? rc : er, sn = pos ? er : rc;      // sigmoid(u) and sigmoid(-u), neither by subtraction
        // log1p(e) from the full-accuracy log and a true division, as in the negative-binomial link
        const bool tiny = t == 1.0f;
        const float lp = logf(t) * (e / (tiny ? 1.0f : t - 1.0f)) + (tiny ? e : 0.0f);
        const float em = -bsc_expm1_f32(-mu);                    // 1 - e^{-mu}, every digit at small mu
        // the branch as an indicator on the input (z0 = 1 on a zero row, zp = 1 on a positive one) that multiplies both
        // branches' terms, as delta does in the Weibull link: a select between the results becomes a branch around the
        // zero row's evaluation, which splits the loop body and spills 140 bytes per lane
        const float z0 = yq == 0.0f ? 1.0f : 0.0f;
        const float zp = 1.0f - z0;
        const float lp0 = fmaxf(dp->tau, -mu) + lp;
        const float lpp = fmaf(yq, lq, -mu);
        const float res = fmaf(-mu, fmaf(z0, sn, zp), yq);
        const float dt0 = su * (1.0f - dp->psi) * em;
        ell = fmaf(vq, fmaf(z0, lp0, zp * lpp) - dp->lg, ell);
        *T = fmaf(vq, fmaf(z0, dt0, -zp * dp->psi), *T);
        return vq * res;
    }
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv) {
        predict_slots3(gp, s, lv);
        const double t = (double)lv, e = exp(-fabs(t));
        gp[2 * P_MAX_S + s] = (float)((t >= 0.0 ? 1.0 : e) / (1.0 + e));
        gp[3 * P_MAX_S + s] = (float)(fmax(t, 0.0) + log1p(e));
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        const float el = expf(l);
        const float q = (1.0f - iv) * el;
        mu = q;
        v = fmaf(q * iv, el, q);
        const float u = lv + el;
        const float e = expf(-fabsf(u));
        const float t = 1.0f + e;
        const float l1p = t == 1.0f ? e : logf(t) * e / (t - 1.0f);
        lp = (yv == 0.0f ? fmaxf(lv, -el) + l1p : fmaf(yv, l, -el)) - lgp;
    }
};

// ---- Student-t: tau = log(1 / sigma), the log of the INVERSE scale, as in the log-normal family; nu > 0, the degrees of
// freedom, is a constant of the MODEL and rides with every launch as one more kernel argument (PARAM); internal ids:
// csrc/bsc_glm_studentt.hip (bsc_studentt_predict_pass) ----------------------------------------------------------------
// glm_disp: (tau, k = 1 / sigma = e^tau, tau + c_nu, nu) with c_nu = lnGamma((nu + 1) / 2) - lnGamma(nu / 2) -
// log(nu pi) / 2 made once per launch in float64 from the float32 nu the kernel was handed, added to tau there and
// rounded once.  y any finite float, l the LOCATION, z = k (y - l):
//     ell  += v [ tau + c_nu - ((nu + 1) / 2) log1p(z^2 / nu) ]                    (the full density, nothing left out)
//     resid = v k (nu + 1) z / (nu + z^2)                                 (= d / d l; BOUNDED in z: the robustness)
//     T    += v nu (1 - z^2) / (nu + z^2)                                 (= d / d tau; not 1 - (nu + 1) z^2 / (nu + z^2),
//                                                                          which cancels near z^2 = 1)
// log1p(r), r = z^2 / nu, through the quotient form log(t) r / (t - 1), t = 1 + r, with the full-accuracy log and a true
// division (t == 1: r itself): the quotient undoes the rounding of t, so that at nu = 1e6, where r is 1e-6 z^2 and the
// product with (nu + 1) / 2 is z^2 / 2, every digit is kept.  1 / nu is a correctly rounded division, the same for every
// row; the two derivatives share one hardware reciprocal of nu + z^2.  NOT clamped and nothing to clamp: every term is
// finite while z^2 is (|z| < 1.8e19), outliers at |z| = 1e4 included.  One log and one reciprocal (and the quotient's
// division) per (row, draw).  A non-finite y on a kept row is the caller's to keep out.
// Prediction: slots (tau + c_nu, k, nu / ((nu - 2) k^2), nu), the first and the third made once per launch in float64 (the
// exp(-logvar) slot carries the variance, +infinity for nu <= 2).  mu = l -- the location: the mean for nu > 1, the
// median always --, v = the third slot; log p in the training forms.
struct StudentT : ScalarFamily {
    static constexpr int GLM_ID = 8, PREDICT_ID = 10;
    static constexpr bool UPPER = false;
    static constexpr bool PARAM = true;            // nu: the last argument of the scalar_par_* kernels
    static __device__ __forceinline__ double log_norm(double nu) {
        return bsc_lgamma_f64(0.5 * (nu + 1.0)) - bsc_lgamma_f64(0.5 * nu) - 0.5 * log(nu * 3.14159265358979323846);
    }
    static __device__ __forceinline__ GlmDisp glm_disp(const float* __restrict__ logphi, int s, int S, float nu) {
        GlmDisp d = glm_disp_tau(logphi, s, S);
        d.lg = (float)((double)d.tau + log_norm((double)nu));
        d.psi = nu;
        return d;
    }
    template <bool OBS, bool ITV>
    static __device__ __forceinline__ float glm_link(float l, float yv, bool real_row, float& ell, float vv,
                                                     const GlmDisp* dp, float* T, float uv) {
        // a dropped row is evaluated at y = 0, l = 0 -- z = 0, every term finite whatever y held (NaN and infinity
        // included)
        const bool keep = real_row && vv > 0.0f;
        const float vq = keep ? vv : 0.0f;
        const float yq = keep ? yv : 0.0f;
        const float lq = keep ? l : 0.0f;
        const float nu = dp->psi;
        const float np1 = nu + 1.0f;
        const float z = dp->phi * (yq - lq);
        const float zz = z * z;
        const float r = zz * (1.0f / nu);
        const float t = 1.0f + r;
        // (t == 1: log(t) = 0 and the quotient is over 1, r itself is added -- selects between values at hand)
        const bool tiny = t == 1.0f;
        const float lp = logf(t) * (r / (tiny ? 1.0f : t - 1.0f)) + (tiny ? r : 0.0f);
        const float q = __builtin_amdgcn_rcpf(fmaf(z, z, nu));
        ell = fmaf(vq, fmaf(-0.5f * np1, lp, dp->lg), ell);
        *T = fmaf(vq, (nu * (1.0f - zz)) * q, *T);
        return vq * ((dp->phi * np1) * (z * q));
    }
    static __device__ __forceinline__ void predict_slots(float* gp, int s, float lv, float nu) {
        predict_slots3(gp, s, lv);
        const double n = (double)nu, k = (double)expf(lv);
        gp[s] = (float)((double)lv + log_norm(n));
        gp[2 * P_MAX_S + s] = nu > 2.0f ? (float)(n / ((n - 2.0) * k * k)) : INFINITY;
        gp[3 * P_MAX_S + s] = nu;
    }
    template <bool ITV>
    static __device__ __forceinline__ void predict_link(float l, float yv, float uv, float lv, float ev, float iv,
                                                        float& mu, float& v, float& lp, float lgp) {
        mu = l;
        v = iv;
        const float z = ev * (yv - l);
        const float r = z * z * (1.0f / lgp);
        const float t = 1.0f + r;
        const float l1p = t == 1.0f ? r : logf(t) * r / (t - 1.0f);
        lp = fmaf(-0.5f * (lgp + 1.0f), l1p, lv);
    }
};

// ---- the ids to the structs ------------------------------------------------------------------------------------------
template <int ID, class... Fs>
struct FamilyById {
    using glm = void;
    using predict = void;
};
template <int ID, class F, class... Fs>
struct FamilyById<ID, F, Fs...> {
    using glm = std::conditional_t<F::GLM_ID == ID, F, typename FamilyById<ID, Fs...>::glm>;
    using predict = std::conditional_t<F::PREDICT_ID == ID, F, typename FamilyById<ID, Fs...>::predict>;
};
template <int ID>
using FamilyOf =
    FamilyById<ID, Logistic, Poisson, Gaussian, NegBin, Gamma, Weibull, Beta, LogNormal, ZeroInflPoisson, StudentT,
               Ordinal>;
template <int LINK>
using GlmFamily = typename FamilyOf<LINK>::glm;
template <int FAM>
using PredictFamily = typename FamilyOf<FAM>::predict;

// The one call of a training pass into a family's link: the row as the struct the pass filled.
template <class F, bool OBS, bool ITV>
__device__ __forceinline__ float glm_link(float l, const GlmRow& r, float& ell, const GlmDisp* dp, float* T) {
    static_assert((!F::SCALAR || OBS) && (!ITV || F::UPPER), "a scalar rides with OBS; the upper end belongs to Weibull");
    return F::template glm_link<OBS, ITV>(l, r.y, r.real, ell, r.v, dp, T, r.u);
}

// The public BSC_SCALAR_* id to its family: f(F{}) with the struct as the argument's type.
inline bool scalar_family_ok(int32_t family) {
    return family == NegBin::SCALAR_ID || family == Gamma::SCALAR_ID || family == Weibull::SCALAR_ID;
}
template <class Fn>
void with_scalar_family(int32_t family, Fn f) {
    if (family == NegBin::SCALAR_ID) f(NegBin{});
    else if (family == Gamma::SCALAR_ID) f(Gamma{});
    else f(Weibull{});
}

}  // namespace
