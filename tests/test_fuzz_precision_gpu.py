"""Random expression trees (test_fuzz_gpu.Grower) through the device executor in float64, in mixed float32 / float64,
and over extents that cross the kernels' vector, workgroup and tile boundaries -- against the float64 numpy oracle.

test_fuzz_gpu.py grows float32 trees over extents <= 7: it never reaches the 16-byte vector paths, the multi-workgroup
reductions, GEMV / split-K, the skinny and stream-K edge tiles or the GEMM prologue / epilogue folds, and it cannot see a
float32 step inside a float64 evaluation.  The families here add the special functions as well (gammaln, digamma, and
the pow(., 0.5), pow(., -1), pow(., 2) that apply_unary in csrc/bsc_fused.hip special-cases), on arguments kept in
(0.25, 3.25] by exp(-|a|).

Tolerances: float64 trees 1e-11 of the result's largest magnitude (a float64 contraction of a few hundred terms and a
chain of libm calls is ~1e-14; one float32 step anywhere is ~1e-7, four orders of magnitude over); trees with any
float32 input are float32 arithmetic and keep test_fuzz_gpu's 2e-4.  A tree whose oracle value is not finite (exp of a
large sum) is grown again from the next seed of its family, so that every case compares numbers."""
import builtins

import numpy as np
import pytest

from bayesic_amd import algebra as A
from bayesic_amd.distribution.special import digamma, gammaln
from oracle.einsum_eval import NumpyBackend
from test_fuzz_gpu import Grower

pytestmark = pytest.mark.gpu

SMALL = {"X": (5, 7), "Y": (5, 7), "Z": (7, 4), "Q": (6, 6), "x": (7,), "y": (5,), "T": (3, 5, 7)}
EDGE = (1, 3, 4, 5, 63, 64, 65, 127, 129, 257)


class PrecisionGrower(Grower):
    """Grower over chosen shapes and declared dtypes, with the special functions as one more operator family."""

    def __init__(self, seed, shapes, dtypes):
        self.rs = np.random.RandomState(seed)
        self.pool = [(A.var(n, len(s), dtypes[n]), s) for n, s in shapes.items()]

    def step(self):
        if self.rs.randint(5):
            return Grower.step(self)
        e, s = self.pick()
        arg = A.exp(-abs(e)) * 3.0 + 0.25                   # in (0.25, 3.25]
        f = [gammaln, digamma, lambda a: A.pow(a, 0.5), lambda a: A.pow(a, -1.0), lambda a: A.pow(e, 2.0)]
        return f[self.rs.randint(len(f))](arg), s


def _edge_shapes(rs):
    m, k, n, q = (int(EDGE[rs.randint(len(EDGE))]) for _ in range(4))
    t = int((1, 3, 5)[rs.randint(3)])
    return {"X": (m, k), "Y": (m, k), "Z": (k, n), "Q": (q, q), "x": (k,), "y": (m,), "T": (t, m, k)}


def _case(family, seed):
    """(expr, inputs, oracle value, declared dtypes) of a tree with a finite oracle value."""
    for attempt in range(20):
        rs = np.random.RandomState(1000 * seed + attempt + {"f64": 1, "mixed": 2, "edge32": 3, "edge64": 4}[family])
        shapes = _edge_shapes(rs) if family.startswith("edge") else SMALL
        if family in ("f64", "edge64"):
            dtypes = {n: "float64" for n in shapes}
        elif family == "edge32":
            dtypes = {n: "float32" for n in shapes}
        else:
            dtypes = {n: ("float64" if rs.randint(2) else "float32") for n in shapes}
        made = PrecisionGrower(int(rs.randint(2 ** 31)), shapes, dtypes).grow(2 + seed % 7)
        if made is None:
            continue
        expr, _ = made
        vals = {n: rs.uniform(-1.0, 1.0, shapes[n]).astype(dtypes[n]) for n in expr.input_types}
        with np.errstate(all="ignore"):
            want = np.asarray(expr.compile(NumpyBackend(np.float64))(**vals), np.float64)
        if np.all(np.isfinite(want)) and (want.size == 0 or np.abs(want).max() < 1e30):
            return expr, vals, want, dtypes
    raise AssertionError("no tree with a finite value for %s seed %d" % (family, seed))


def _check(ctx, family, seed, rtol):
    from bayesic_amd.algebra.device_backend import DeviceBackend
    expr, vals, want, dtypes = _case(family, seed)
    got = np.asarray(expr.compile(DeviceBackend(ctx))(**vals))
    assert got.shape == want.shape, repr(expr)
    wide = any(dtypes[n] == "float64" for n in expr.input_types)
    if got.ndim:                                            # (a 0-d result may come back as a Python float)
        assert got.dtype == (np.float64 if wide else np.float32), (repr(expr), got.dtype, wide)
    if want.size == 0:
        return
    scale = builtins.max(float(np.abs(want).max()), 1e-3)
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= rtol * scale, "%r: max err %g of scale %g" % (expr, err, scale)


@pytest.mark.parametrize("seed", range(150))
def test_float64_tree_matches_the_oracle_to_float64_accuracy(ctx, seed):
    _check(ctx, "f64", seed, 1e-11)


@pytest.mark.parametrize("seed", range(60))
def test_mixed_dtype_tree_promotes_like_numpy(ctx, seed):
    _check(ctx, "mixed", seed, 2e-4)


@pytest.mark.parametrize("seed", range(50))
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_tree_over_edge_extents(ctx, dtype, seed):
    _check(ctx, "edge32" if dtype == "float32" else "edge64", seed, 2e-4 if dtype == "float32" else 1e-11)
