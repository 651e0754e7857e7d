// digamma and lnGamma in float64, shared by the kernels of libbayesic_hip.so (through bsc_common.h) and built
// for the host as well (tests/test_special_host.py compiles this header alone with the system C++ compiler).
//
// For x > 0 (finite) both shift the argument up to y = x + n >= 8 with n <= 8 steps and evaluate the asymptotic
// series there.  Every other argument takes ONE branch, so the streaming kernels keep the x > 0 code as it was:
//   finite x < 0, not an integer:  reflection, 1 - x > 1 goes through the x > 0 code
//       psi(x)     = psi(1 - x) - pi / tan(pi r)
//       lnGamma(x) = log(pi) - log|sin(pi r)| - lnGamma(1 - x)      (lnGamma = log|Gamma|)
//     with r = x - rint(x) in [-1/2, 1/2] (exact), so the period is removed before pi multiplies
//   the special values (scipy.special's conventions for every finite input and for NaN and +inf):
//       psi(+0) = -inf, psi(-0) = +inf, psi(negative integer) = NaN, psi(-inf) = NaN, psi(+inf) = +inf,
//       lnGamma(+-0) = +inf, lnGamma(negative integer) = +inf, lnGamma(+-inf) = +inf, NaN -> NaN.
//     (scipy's gammaln(-inf) is -inf; here it is C99 lgamma's +inf, |Gamma| having no limit there.)
// Every finite x <= -2^52 is an integer, so no argument ever reaches a loop that cannot end: `x += 1.0` leaves
// x unchanged from -2^53 down, which once made `while (x < 8) x += 1` spin forever on -inf or -1e300.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define BSC_HD __host__ __device__
#else
#define BSC_HD
#endif

constexpr double BSC_PI = 3.14159265358979323846264338327950288;
constexpr double BSC_LOG_PI = 1.14472988584940017414342735135305871;
constexpr double BSC_LOG_2PI = 1.8378770664093454835606594728112;

// digamma: recurrence up to x >= 8, then the asymptotic series
//   ln x - 1/2x - 1/12x^2 + 1/120x^4 - 1/252x^6 + 1/240x^8 - 5/660x^10 + 691/32760x^12 - 1/12x^14
// (next term 3617/8160x^16 < 2e-15 at x = 8; without the x^14 term the error was 1/12x^14 ~ 2e-14, 1e-13
// relative next to the root at 1.4616).  Shared by the Dirichlet / Normal-Gamma expectations and the
// element-wise digamma of the executor.
BSC_HD inline double bsc_digamma_f64(double x) {
#pragma clang fp contract(off)
    double refl = 0.0;
    if (!(x > 0.0)) {                       // x <= 0, -inf, NaN: the one slow branch
        if (x == 0.0) return copysign(INFINITY, -x);
        const double r = x - rint(x);       // NaN for x = -inf and x = NaN
        if (!(r != 0.0)) return NAN;        // negative integers, -inf, NaN
        refl = -BSC_PI / tan(BSC_PI * r);
        x = 1.0 - x;
    }
    // shift x up to >= 8: psi(x) = psi(x + n) - sum_{i<n} 1/(x + i).  The sum is P'(x)/P(x) for
    // P = prod (x + i), built with multiplies and adds, so it costs ONE division instead of n
    // (float64 division is ~10x a multiply; this halves bsc_dirichlet_expectation).  x > 0 here:
    // at most 8 steps (+inf: none)
    double P = 1.0, dP = 0.0;
    while (x < 8.0) {
        dP = dP * x + P;
        P *= x;
        x += 1.0;
    }
    const double acc = -dP / P;
    const double inv = 1.0 / x, inv2 = inv * inv;
    const double series = inv2 * (1.0 / 12.0 - inv2 * (1.0 / 120.0 - inv2 * (1.0 / 252.0 - inv2 *
                          (1.0 / 240.0 - inv2 * (5.0 / 660.0 - inv2 * (691.0 / 32760.0 - inv2 * (1.0 / 12.0)))))));
    return acc + log(x) - 0.5 * inv - series + refl;
}

// lnGamma in float64 by the same route: lnGamma(x) = lnGamma(x + n) - log prod_{i<n} (x + i), x + n >= 8,
// Stirling's series there, up to the 1 / (156 y^13) term (the next, 3617 / (122400 y^15), is < 1e-15 at y = 8).
BSC_HD inline double bsc_lgamma_f64(double x) {
#pragma clang fp contract(off)
    double refl = 0.0, sign = 1.0;
    if (!(x > 0.0 && x < INFINITY)) {       // x <= 0, +-inf, NaN: the one slow branch
        if (x != x) return x;
        if (x == 0.0 || x == INFINITY || x == -INFINITY) return INFINITY;
        const double r = x - rint(x);
        if (r == 0.0) return INFINITY;      // the poles at the negative integers
        refl = BSC_LOG_PI - log(fabs(sin(BSC_PI * r)));
        sign = -1.0;
        x = 1.0 - x;
    }
    double P = 1.0;
    while (x < 8.0) {                       // x > 0 here: at most 8 steps
        P *= x;
        x += 1.0;
    }
    const double inv = 1.0 / x, inv2 = inv * inv;
    const double series = inv * (1.0 / 12.0 - inv2 * (1.0 / 360.0 - inv2 * (1.0 / 1260.0 - inv2 *
                          (1.0 / 1680.0 - inv2 * (1.0 / 1188.0 - inv2 * (691.0 / 360360.0 - inv2 * (1.0 / 156.0)))))));
    const double lg = (x - 0.5) * log(x) - x + 0.91893853320467274178032973640562 + series - log(P);
    return refl + sign * lg;
}
