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
// bsc_glm_nb_data_pass).  Device only, header-only, internal linkage.
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

}  // namespace
