// lnGamma and digamma differences in float32 for the lanes of the negative-binomial passes (csrc/bsc_glm_nb.hip):
//     dlnGamma(y, phi) = lnGamma(y + phi) - lnGamma(phi),     dpsi(y, phi) = psi(y + phi) - psi(phi),     y >= 0, phi > 0
// from lg0 = lnGamma(phi) and ps0 = psi(phi), which the caller makes once per draw (in float64, csrc/bsc_special.h).
// Both routes are ONE product of at most eight factors, P = prod_{i<n} (a + i), carried with its derivative P' so that
// it costs one log (lnGamma) and one reciprocal (psi) -- straight-line selects, no loop a lane could diverge in:
//   y a whole number up to 8 (what counts mostly are):  a = phi, n = y.  The differences ARE the product and the sum,
//       dlnGamma = log P,   dpsi = P' / P
//     exactly 0 at y = 0 and good to a few ulps of the RESULT.  (Through the route below every row with the same small
//     count carries the same error of a few ulps of the shifted Stirling term, ~16: rows do not average it away, and
//     it showed in the ELBO at 2e-6.)
//   otherwise:  a = z = y + phi, n = the steps that shift z up to z + n >= 8 (none for y > 8), then three asymptotic
//     terms there (the fourth is below 1e-9 at 8):
//       dlnGamma = Stirling(z + n) - log P - lg0,   dpsi = asymptotic(z + n) - P' / P - ps0
//     with an absolute error of a few ulps of the largest term, (z - 1/2) log z.
// The route is chosen by selects on the INPUTS of the product; its two results are combined with factors 0 / 1 and
// +1 / -1, all finite, so that the compiler has no expensive operand to branch around.
// Callers state the range of phi over which the differences are good enough (include/bayesic_hip.h,
// bsc_glm_nb_data_pass).  bsc_lgamma_psi_f32 below is the pair itself, not a difference, for any positive argument (the
// Beta link); bsc_lognormsf_hazard_f32 at the end is the normal log survival function and hazard (the log-normal link).
// Device only, header-only, internal linkage.
#pragma once

namespace {

__device__ __forceinline__ void bsc_dlgamma_dpsi_f32(float y, float phi, float lg0, float ps0, float& dlg, float& dps) {
    const float z = y + phi;
    const bool count = y <= 8.0f && y == floorf(y);
    const float a = count ? phi : z;
    const float n = count ? y : 8.0f - z;          // factors a + i for i < n
    float P = 1.0f, dP = 0.0f, zz = a;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool take = (float)i < n;
        const float f = a + (float)i;
        dP = take ? fmaf(dP, f, P) : dP;
        P = take ? P * f : P;
        zz = take ? f + 1.0f : zz;                 // the shifted argument (not used by the count route)
    }
    const float lP = logf(P);
    const float q = dP * __builtin_amdgcn_rcpf(P);
    const float lz = logf(zz);
    const float inv = __builtin_amdgcn_rcpf(zz), inv2 = inv * inv;
    const float stirling = fmaf(zz - 0.5f, lz, -zz) + 0.91893853320467274f +
                           inv * (1.0f / 12.0f - inv2 * (1.0f / 360.0f - inv2 * (1.0f / 1260.0f)));
    const float asym = lz - 0.5f * inv - inv2 * (1.0f / 12.0f - inv2 * (1.0f / 120.0f - inv2 * (1.0f / 252.0f)));
    const float on = count ? 0.0f : 1.0f, sgn = count ? 1.0f : -1.0f;
    dlg = fmaf(on, stirling - lg0, sgn * lP);
    dps = fmaf(on, asym - ps0, sgn * q);
}

// lnGamma(x) and psi(x) together for ANY float32 x > 0 (the Beta link, csrc/bsc_glm_beta.hip, whose two arguments
// m phi and (1 - m) phi change with every (row, draw) and run towards 0 as the logit grows): the "otherwise" route above
// without its subtraction.  n = the steps that shift x up to x + n >= 8 (none for x >= 8), ONE product P = prod_{i<n}
// (x + i) of at most eight factors carried with P', three asymptotic terms at x + n:
//     lnGamma = Stirling(x + n) - log P,     psi = asymptotic(x + n) - P' / P
// Straight-line, the selects on the inputs of the product; two logs and two reciprocals.  Absolute error: a few ulps of
// the largest term formed -- the shifted Stirling term (~10.6 at 8, (x - 1/2) log x above) or |log x| and 1 / x below 1,
// where lnGamma ~ -log x and psi ~ -1 / x carry their own relative rounding and no more.  Finite while P and 1 / P are:
// x > 1e-37 (P ~ 5040 x, P' / P ~ 1 / x).  The psi half folds away where it is not used.
__device__ __forceinline__ void bsc_lgamma_psi_f32(float x, float& lg, float& ps) {
    const float n = 8.0f - x;                      // factors x + i for i < n
    float P = 1.0f, dP = 0.0f, zz = x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool take = (float)i < n;
        const float f = x + (float)i;
        dP = take ? fmaf(dP, f, P) : dP;
        P = take ? P * f : P;
        zz = take ? f + 1.0f : zz;                 // the shifted argument
    }
    const float lz = logf(zz);
    const float inv = __builtin_amdgcn_rcpf(zz), inv2 = inv * inv;
    const float stirling = fmaf(zz - 0.5f, lz, -zz) + 0.91893853320467274f +
                           inv * (1.0f / 12.0f - inv2 * (1.0f / 360.0f - inv2 * (1.0f / 1260.0f)));
    const float asym = lz - 0.5f * inv - inv2 * (1.0f / 12.0f - inv2 * (1.0f / 120.0f - inv2 * (1.0f / 252.0f)));
    lg = stirling - logf(P);
    ps = fmaf(-dP, __builtin_amdgcn_rcpf(P), asym);
}

// Interval censoring (csrc/bsc_families.h: Weibull's glm_link_upper and predict_link_upper, ONE value for
// the training pass and the predictive): from Delta = ITV_BIG on the upper end of a row is read as absent.
constexpr float ITV_BIG = 103.0f;              // e^{-103} = 1.8e-45: at most one denormal step from 1 - e^{-Delta} = 1

// expm1 from the full-accuracy exp and log: u - 1 with u = e^x where that does not cancel (|x| > 1/2), else Kahan's
// (u - 1) x / log u, which undoes the rounding of u (u - 1 is exact there), and x itself where u == 1.  The selects sit
// on the inputs of the quotient (a select on its result turns into a branch around it); e^x infinite gives infinity.
__device__ __forceinline__ float bsc_expm1_f32(float x) {
    const float u = expf(x);
    const bool far = fabsf(x) > 0.5f, one = u == 1.0f;
    const float lu = logf(one ? 2.0f : u);                       // never 0 where it divides
    return fmaf(u - 1.0f, (far ? 1.0f : x) * __builtin_amdgcn_rcpf(far ? 1.0f : lu), one ? x : 0.0f);
}

// log(b / a) for b >= a > 0, la = log a at hand.  b < 2 a: b - a is exact and log1p((b - a) / a) keeps every digit of a
// narrow ratio (the difference of two rounded logarithms loses |log a| eps of it) -- log1p(r) = log(w) r / (w - 1) with
// w = 1 + r, the quotient undoing the rounding of w, and r itself where w == 1; else log b - la.  ONE logarithm, the
// selects on its input and between values at hand; exactly 0 at b == a.
__device__ __forceinline__ float bsc_logratio_f32(float b, float a, float la) {
    const bool near = b < 2.0f * a;
    const float r = (near ? b - a : 0.0f) * __builtin_amdgcn_rcpf(a);
    const float w = 1.0f + r;
    const bool one = w == 1.0f;
    const float lg = logf(near ? w : b);
    const float ratio = near ? r * __builtin_amdgcn_rcpf(one ? 1.0f : w - 1.0f) : 1.0f;
    return fmaf(lg, ratio, one ? r : 0.0f) - (near ? 0.0f : la);
}

// erfcx(a) = e^{a^2} erfc(a) for a finite a >= 0, in (0, 1], straight-line (with the library's erfcxf, which serves
// negative arguments too, the 8-row pass of the log-normal link spills 140 bytes per lane; with this one it keeps 233
// registers and no scratch).  The half line is mapped to t = (a - 2) / (a + 2) in [-1, 1), where
// (1 + 2 a) erfcx(a) - 1 is smooth up to its limit 2 / sqrt(pi) - 1 at t = 1: a polynomial of degree 11 in t
// (interpolated at the Chebyshev nodes in float64 against a float64 erfcx, 1.9e-8 off at most, rounded to float32), then
// the division by 1 + 2 a.  Both quotients are a reciprocal with ONE correction step from their exact residuals (fmaf),
// so neither costs more than a rounding.  Within 1.8 float32 roundings of erfcx over [0, 1e19]:
// tests/test_glm_lognormal_cpu.py replays these steps and these coefficients in float32 on the host
// (tests/_glm_lognormal_ref.erfcx_pos_f32).
__device__ __forceinline__ float bsc_erfcx_pos_f32(float a) {
    const float r2 = __builtin_amdgcn_rcpf(a + 2.0f);
    const float t0 = (a - 2.0f) * r2;
    const float t = fmaf(r2, fmaf(t0, -a, fmaf(t0 + 1.0f, -2.0f, a)), t0);     // + r2 ((a - 2) - t0 (a + 2))
    float p = 6.807514728279784e-05f;
    p = fmaf(p, t, 1.6084033995866776e-04f);
    p = fmaf(p, t, -3.709284064825624e-04f);
    p = fmaf(p, t, -1.3958050403743982e-03f);
    p = fmaf(p, t, 1.230503199622035e-03f);
    p = fmaf(p, t, 8.68925265967846e-03f);
    p = fmaf(p, t, -8.024739101529121e-03f);
    p = fmaf(p, t, -5.4211996495723724e-02f);
    p = fmaf(p, t, 1.6405050456523895e-01f);
    p = fmaf(p, t, -1.660310924053192e-01f);
    p = fmaf(p, t, -9.276381880044937e-02f);
    p = fmaf(p, t, 2.7697840332984924e-01f);
    const float r = 0.5f * __builtin_amdgcn_rcpf(a + 0.5f);                    // 1 / (1 + 2 a)
    const float q = fmaf(p, r, r);
    return fmaf((p - q) + fmaf(q + q, -a, 1.0f), r, q);                        // + r ((1 + p) - q (1 + 2 a))
}

// The log survival function and the hazard of the standard normal together, for any finite float32 z with z^2 finite
// (the log-normal link's censored rows, csrc/bsc_glm_lognormal.hip):
//     lsf = log Phi(-z),     hz = phi(z) / Phi(-z)
// from ONE scaled complementary error function E = erfcx(|z| / sqrt 2) in (0, 1] (bsc_erfcx_pos_f32 above), which
// neither tail can overflow or cancel, and g = e^{-z^2 / 2} (the exponential of the ROUNDED square times one minus the
// square's rounding error, which an fmaf gives exactly: without it g is off by z^2 / 2 roundings, 32 at z = -13):
//   z >= 0:  Phi(-z) = g E / 2, so    lsf = -z^2 / 2 + log(E / 2),     hz = sqrt(2 / pi) / E       (g itself is not used:
//            at z = 60 it is 0 in float32 and lsf = -1805.01 all the same)
//   z <  0:  q = Phi(z) = g E / 2 in (0, 1/2), so    lsf = log1p(-q),     hz = phi(z) / (1 - q)
//            with log1p(-q) = log(w) q / (1 - w), w = 1 - q in [1/2, 1): 1 - w is exact and the quotient undoes the
//            rounding of w; -q itself where w == 1.  hz runs to 0 with g.
// The one form -z^2 / 2 + log(E(z) / 2) for every z would lose the left tail to cancellation (both terms ~ z^2 / 2, the
// result ~ -q).  ONE log and ONE reciprocal, the selects on their inputs and between values at hand; both results within
// a few roundings of max(|lsf|, z^2 / 2) and of hz.  The hz half folds away where it is not used.
__device__ __forceinline__ void bsc_lognormsf_hazard_f32(float z, float& lsf, float& hz) {
    const bool pos = z >= 0.0f;
    const float E = bsc_erfcx_pos_f32(fabsf(z) * 0.70710678118654752f);
    const float hz2 = 0.5f * z * z;
    const float g0 = expf(-hz2);
    const float g = fmaf(-g0, fmaf(0.5f * z, z, -hz2), g0);    // e^{-(hz2 + d)} = g0 (1 - d), d the rounding of hz2
    const float q = 0.5f * g * E;
    const float w = 1.0f - q;
    const bool tiny = !pos && w == 1.0f;
    const float lg = logf(pos ? 0.5f * E : w);
    const float ratio = pos ? 1.0f : q * __builtin_amdgcn_rcpf(tiny ? 1.0f : 1.0f - w);
    const float add0 = pos ? -hz2 : 0.0f;
    lsf = fmaf(lg, ratio, tiny ? -q : add0);
    hz = (pos ? 0.79788456080286536f : 0.39894228040143268f * g) * __builtin_amdgcn_rcpf(pos ? E : w);
}

}  // namespace
