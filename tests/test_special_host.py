"""bsc_digamma_f64 / bsc_lgamma_f64 (csrc/bsc_special.h, included by every kernel through bsc_common.h) built for the
HOST from the very header the kernels compile, and evaluated over the whole float64 line against scipy.

The arguments that once made the shift loop `while (x < 8) x += 1` spin forever (-inf, every finite x <= -2^53,
where x + 1 == x) and those that made it run for seconds (-1e9) are evaluated here, on the CPU, in a child process
under a time limit: a regression fails this test by timeout instead of hanging the suite or a GPU.  No GPU test
sends such an argument to the device.

Tolerances.  x > 0: the series at y >= 8 is accurate to < 1e-15 absolute, the shift adds at most eight rounded
products and one quotient, so 1e-13 relative holds with room; near the zero of digamma (x ~ 1.4616) and those of
lnGamma (x = 1, 2) the result is a difference of O(1) terms (log y ~ 2, log P ~ 8), so an absolute 2e-15 resp.
2e-14 joins the relative bound.  x < 0 (reflection): the error is relative to the two terms that are added
(psi(1 - x) and pi cot(pi x), resp. log pi - log|sin(pi x)| and lnGamma(1 - x)), so the bound is 1e-13 of the
sum of their magnitudes -- the condition of the sum, which is large only next to the roots between the poles."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import special

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bayesic_amd", "csrc", "bsc_special.h")

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "bsc_special.h"
// reads doubles from stdin, writes psi(x) and lnGamma(x) for each (binary, two doubles per argument)
int main() {
    std::vector<double> x;
    double v;
    while (std::fread(&v, sizeof v, 1, stdin) == 1) x.push_back(v);
    for (double a : x) {
        const double r[2] = {bsc_digamma_f64(a), bsc_lgamma_f64(a)};
        std::fwrite(r, sizeof r[0], 2, stdout);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("special_host")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    # strict IEEE: no contraction, no fast-math (the kernels build these functions with fp contract off)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                           "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)])
    return str(exe)


def evaluate(driver, x):
    x = np.ascontiguousarray(x, np.float64)
    try:
        run = subprocess.run([driver], input=x.tobytes(), stdout=subprocess.PIPE, timeout=60, check=True)
    except subprocess.TimeoutExpired:
        pytest.fail("bsc_digamma_f64 / bsc_lgamma_f64 did not return within 60 s for %d arguments: a shift loop "
                    "that does not end" % x.size)
    out = np.frombuffer(run.stdout, np.float64).reshape(-1, 2)
    assert out.shape[0] == x.size
    return out[:, 0], out[:, 1]


def test_special_values_end_and_follow_the_documented_conventions(driver):
    inf, nan = math.inf, math.nan
    # (x, psi, lnGamma): scipy's values, except lnGamma(-inf) = +inf (C99 lgamma; scipy says -inf)
    cases = [(0.0, -inf, inf), (-0.0, inf, inf), (inf, inf, inf), (-inf, nan, inf), (nan, nan, nan),
             (-1.0, nan, inf), (-2.0, nan, inf), (-1e9, nan, inf), (-2.0 ** 53, nan, inf), (-2.0 ** 52, nan, inf),
             (-1e300, nan, inf), (-np.finfo(np.float64).max, nan, inf)]
    x = np.array([c[0] for c in cases])
    psi, lg = evaluate(driver, x)
    for (v, want_psi, want_lg), p, g in zip(cases, psi, lg):
        for got, want, name in ((p, want_psi, "psi"), (g, want_lg, "lnGamma")):
            if math.isnan(want):
                assert math.isnan(got), (name, v, got)
            else:
                assert got == want, (name, v, got, want)
    # every finite argument above is scipy's convention too
    for v, p, g in zip(x, psi, lg):
        if np.isfinite(v):
            np.testing.assert_equal(p, special.digamma(v))
            np.testing.assert_equal(g, special.gammaln(v))


def test_subnormal_and_huge_arguments(driver):
    x = np.array([1e-310, 5e-324, 1e-300, 1e300, np.finfo(np.float64).max])
    psi, lg = evaluate(driver, x)
    # psi(x) = -1/x - euler + O(x): -inf once 1/x overflows
    assert psi[0] == -math.inf and psi[1] == -math.inf
    assert abs(psi[2] - (-1e300)) <= 1e-15 * 1e300
    # lnGamma(x) = -log x - euler x + O(x^2) (scipy's gammaln overflows to inf for subnormal x)
    for i in (0, 1, 2):
        assert abs(lg[i] - (-math.log(x[i]))) <= 1e-13 * abs(lg[i]), (x[i], lg[i])
    np.testing.assert_allclose(psi[3:], special.digamma(x[3:]), rtol=1e-13)
    np.testing.assert_allclose(lg[3], special.gammaln(x[3]), rtol=1e-13)
    assert lg[4] == math.inf or abs(lg[4] - special.gammaln(x[4])) <= 1e-13 * special.gammaln(x[4])


def test_positive_arguments_match_scipy_to_float64_accuracy(driver):
    grid = np.logspace(-300, 300, 1201)
    dense = np.linspace(1e-3, 20.0, 4001)                      # the shift region and the start of the series
    roots = np.array([1.4616321449683623, 1.0, 2.0, 1.0 + 2 ** -40, 2.0 - 2 ** -40])
    x = np.concatenate([grid, dense, roots, [8.0, 8.0 - 2 ** -49, 7.5, 0.5]])
    psi, lg = evaluate(driver, x)
    want_psi, want_lg = special.digamma(x), special.gammaln(x)
    bad = ~(np.abs(psi - want_psi) <= 1e-13 * np.abs(want_psi) + 2e-15)
    assert not bad.any(), list(zip(x[bad][:5], psi[bad][:5], want_psi[bad][:5]))
    bad = ~(np.abs(lg - want_lg) <= 1e-13 * np.abs(want_lg) + 2e-14)
    assert not bad.any(), list(zip(x[bad][:5], lg[bad][:5], want_lg[bad][:5]))


def test_negative_non_integers_by_reflection(driver):
    rs = np.random.RandomState(7)
    frac = rs.uniform(0.02, 0.98, 600)
    whole = -np.floor(np.logspace(0, 15, 600))                 # down to -1e15 (the fraction is still resolved)
    x = np.concatenate([whole + frac - 1.0, [-2.5, -0.5, -1e-300, -1e9 + 0.5, -0.999, -1.001, -4.2e7 + 0.25]])
    x = x[x != np.rint(x)]                                     # (near 1e15 a fraction can round away: a pole)
    assert x.size > 550
    psi, lg = evaluate(driver, x)
    want_psi, want_lg = special.digamma(x), special.gammaln(x)
    r = x - np.rint(x)
    scale_psi = np.abs(special.digamma(1.0 - x)) + np.abs(math.pi / np.tan(math.pi * r))
    bad = ~(np.abs(psi - want_psi) <= 1e-13 * scale_psi)
    assert not bad.any(), list(zip(x[bad][:5], psi[bad][:5], want_psi[bad][:5]))
    scale_lg = math.log(math.pi) + np.abs(np.log(np.abs(np.sin(math.pi * r)))) + np.abs(special.gammaln(1.0 - x))
    bad = ~(np.abs(lg - want_lg) <= 1e-13 * scale_lg)
    assert not bad.any(), list(zip(x[bad][:5], lg[bad][:5], want_lg[bad][:5]))


def test_the_kernels_include_this_header():
    """The functions tested here are the kernels' own: bsc_common.h includes bsc_special.h and keeps no copy."""
    common = open(os.path.join(ROOT, "bayesic_amd", "csrc", "bsc_common.h")).read()
    assert '#include "bsc_special.h"' in common
    assert "bsc_digamma_f64(double" not in common and "bsc_lgamma_f64(double" not in common
