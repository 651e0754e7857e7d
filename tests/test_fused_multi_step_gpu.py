"""The fused map and reduce kernels of csrc/bsc_fused.hip where one wave or thread takes SEVERAL steps of its outer loop
(grid-stride sweeps, persistent row steps, interleaved split pieces) and where the second level runs (four waves folded
through LDS, split partials folded by map_reduce_finish_kernel).  Every other GPU test of these kernels stops at one
step, or reaches a second one on a shape where the step is a no-op (tests/test_fusion_gpu.py, test_view_routes_gpu.py).

Shapes come from the device.  tests/_fused_plan.py restates the dispatcher's host arithmetic; every run first asserts,
with the device's own cu_count, the kernel and the steps or splits its case was built for.  The steps are pulled down to
a few MB by three per-context options: a second Context (the `alt` fixture) with rows_wg, fused_map_blocks_per_cu or
fused_waves_per_cu at 1.  tests/test_fused_plan_cpu.py checks the tables at 64, 256 and 304 CUs.

Buffers are tests/_views.py's: every output lies in a buffer of one NaN bit pattern with 64 guard elements before and
after it (and in the gaps of a strided output) that must not change; every input is NaN outside its view.

1-5. Exact accounting.  Small integers that depend on their position -- x[o, r] = 1 + (3 o + 5 r + (o r) // 7) mod 7
   (mod 3 for sums above 390 000 terms), riders 1 + (r mod 3) along the reduce axis or 1 + (o mod 3) along the kept
   one, biases c + 1 per column -- combined by `mul`, then scale 0.5 and shift 0.25 (or 1 and 0).  Every value is a
   multiple of 1/4 far below 2^22, so the float32 products, the float64 accumulation, the LDS fold, the split partials
   and the final cast are all exact: the result must be BIT-EQUAL to an int64 reference, and a lost, doubled or
   mis-paired element moves an output by >= 0.75.  Runs of one case under contexts that differ only in an option
   must be bit-equal to each other as well.  Not LINEAR: pow 0.5 on perfect squares and post abs.
   1. map_reduce_rows_f32_kernel, rows_wg = 1: n_out = (k - 1) 16 cu + 21 for k = 2, 3, 5 persistent steps.  (On a
      device with fewer than 256 CUs rows_wg is the smallest value that keeps two steps above the kernel's floor of
      4 096 outputs: `rows_wg_for`.)
   2. map_dense_f32_kernel<2>, fused_map_blocks_per_cu = 1: two sweeps of 512 cu float4 and a ragged third.
   3. the same kernel with a periodic operand (a bias row vector): three sweeps, pstep != 0, the wrap of `prem` runs.
   4. map_rows_f32_kernel: three row steps; four and three column chunks with a narrow last one.
   5. splits > 1 in the five reduce kernels, the finish kernel's four-in-flight loop (splits > 192) and its
      thread-per-output form (n_out >= 4096), the narrow kernel at every L = n_out / 4, dividing 64 or not.
6. Parity on real values with the inputs, ops and tolerances of test_fusion_gpu.test_map_reduce_matches_numpy, one case
   per kernel, against float64 numpy.  (The broadcast operand is one value per row there; the dense map takes a full
   operand and the periodic map a row vector instead, which is what those kernels accept.)
7. Two runs of one case per reduce kernel are bit-identical.

First device run (MI355X, cu_count 256, the shipped kernels unchanged): all 125 tests passed.
  * Every exact case of 1-5 held BIT FOR BIT against the int64 reference and between its contexts: 30 short-row, 4 dense
    map, 10 periodic map, 5 row map and 48 split cases (float64 among them), the pow 0.5 / abs instantiations included.
  * Worst error / bound of 6 (mul, add; each case prints its own under -s): map_reduce_rows 0.0088, 0.0071;
    map_dense 0.021, 0.013; map_dense with a periodic operand 0.024, 0.014; map_rows 0.022, 0.014;
    map_reduce_wave_dense 0.0051, 0.0041; map_reduce_wave 0.0027, 0.0047 (float64 1.2e-4, 2.1e-4);
    map_reduce_lane_dense 0.0055, 0.0044; map_reduce_lane 0.0040, 0.0060 (float64 1.1e-3, 1.3e-3);
    map_reduce_lane_narrow 0.0057, 0.0051.
  * With the wrap of `prem` removed (csrc/bsc_fused.hip:242), 12 tests here fail and no other GPU test does.  With the
    narrow kernel's `rb += splits * step` cut to `rb += step`, 18 fail here -- and 13 older tests, which already sum
    narrow matrices in several splits.  With the short-row loop cut to its first step, 32 fail here and, of the older
    tests, only a route check on a 1M-row model.  Changing that loop's stride to `r0 += n_waves` cannot fail any test
    of results: the wave then visits a superset of its rows and stores every one of them from its own data, so the
    outputs are the same and only the time changes.
"""
import collections
import ctypes
import functools

import numpy as np
import pytest

import _fused_plan as fp
import _views as V

pytestmark = pytest.mark.gpu

OPS = {"add": 0, "mul": 1, "log": 2, "exp": 3, "pow": 4, "abs_": 5, "copy": 6}
COPY = ("copy", 0.0)
HALF, UNIT = (0.5, 0.25), (1.0, 0.0)          # (scale, shift)
F32, F64 = np.float32, np.float64
ROWS, DENSE, FLAT, ROWMAP = ("map_reduce_rows_f32_kernel", "map_dense_f32_kernel", "map_flat_f32_kernel",
                             "map_rows_f32_kernel")
WAVE_DENSE, WAVE, LANE_DENSE, LANE, NARROW = ("map_reduce_wave_dense_f32_kernel", "map_reduce_wave_kernel",
                                              "map_reduce_lane_dense_f32_kernel", "map_reduce_lane_kernel",
                                              "map_reduce_lane_narrow_f32_kernel")
BLOCKS1, WAVES1, NOFLAT = {"fused_map_blocks_per_cu": 1}, {"fused_waves_per_cu": 1}, {"fused_map_flat": 0}


# ---- cases ----------------------------------------------------------------------------------------------------------

def case(shape, red, operands, runs, affine=HALF, post=COPY, combine="mul", out_inner=1, dtype=F32, seed=None):
    """shape: (N,) or (A, B), the full index space.  red: None (a pure map) or the reduced axis of (A, B).
    operands: (data, pad, pre op) -- `data` names a generator below, whose result's shape says what the operand is: the
    full index space (rows `pad` elements further apart than dense), a row vector (1, B), one value per row (A, 1) or
    one value (1, 1).  runs: [(context options, what the plan must say)], the run the case is named for first.
    seed: real-valued data (parity), else the exact small integers."""
    operands = [o if isinstance(o, tuple) and len(o) == 3 else (o, 0, COPY) for o in operands]
    return dict(shape=tuple(shape), red=red, operands=operands, runs=runs, affine=affine, post=post, combine=combine,
                out_inner=out_inner, dtype=dtype, seed=seed)


def sq(pad=0):
    """x stored as its square and read through pow 0.5: exact, and not one of linear_ops."""
    return ("x7sq", pad, ("pow", 0.5))


def _index_grids(c):
    """(o, r, column): kept and reduced index of every element (for a map: row and column), broadcastable to the
    index space as a 2-D array; a flat array counts as one row whose `o` changes every 61 elements."""
    if len(c["shape"]) == 1:
        i = np.arange(c["shape"][0], dtype=np.int64)[None, :]
        return i // 61, i, i
    A, B = c["shape"]
    i0, i1 = np.arange(A, dtype=np.int64)[:, None], np.arange(B, dtype=np.int64)[None, :]
    return (i1, i0, i1) if c["red"] == 0 else (i0, i1, i1)


def _full(c):
    """The index space as a 2-D shape: a flat array is one row."""
    return (1, c["shape"][0]) if len(c["shape"]) == 1 else c["shape"]


def _x(o, r, m):
    return 1 + (3 * o + 5 * r + (o * r) // 7) % m


def exact_values(c):
    """[(stored, effective)] per operand, int64: what is uploaded, and what the value is after the pre op."""
    o, r, col = _index_grids(c)
    width = c["shape"][-1]
    out = []
    for data, _, pre in c["operands"]:
        if isinstance(data, tuple):
            assert data[0] == "const"
            v = np.full((1, 1), data[1], np.int64)
        else:
            v = {"x7": lambda: _x(o, r, 7), "x3": lambda: _x(o, r, 3), "x7sq": lambda: _x(o, r, 7),
                 "r3": lambda: 1 + r % 3, "r2": lambda: 1 + r % 2, "r5": lambda: 1 + r % 5, "k3": lambda: 1 + o % 3,
                 "bias": lambda: col + 1, "biasr": lambda: width - col}[data]()
        if data == "x7sq":
            assert pre == ("pow", 0.5)
            out.append((v * v, v))
        else:
            assert pre == COPY
            out.append((v, v))
    return out


def exact_reference(c):
    """float64, every entry an exact multiple of 1/4: the int64 sum of 4 (scale * product + shift), divided by 4."""
    assert c["combine"] == "mul" and c["affine"] in (HALF, UNIT) and c["post"] in (COPY, ("abs_", 0.0))
    full = _full(c)
    p = np.ones(full, np.int64)
    for _, eff in exact_values(c):
        p = p * eff
    q4 = 2 * p + 1 if c["affine"] == HALF else 4 * p
    assert q4.min() > 0                                       # post abs changes nothing
    if c["red"] is not None:
        q4 = q4.sum(axis=c["red"])
    elif len(c["shape"]) == 1:
        q4 = q4[0]
    assert q4.dtype == np.int64
    return q4 / 4.0


NP_UNARY = {"copy": lambda x, a: x, "log": lambda x, a: np.log(x), "exp": lambda x, a: np.exp(x),
            "abs_": lambda x, a: np.abs(x), "pow": lambda x, a: np.power(x, a)}


def real_values(c):
    """test_fusion_gpu.test_map_reduce_matches_numpy's inputs: a = U(0.5, 1.5), b = N(0, 1), c = U(0.5, 1.5) broadcast
    (`c_col` one value per row as there, `c_row` a row vector, `c` full)."""
    rng = np.random.RandomState(c["seed"])
    full = _full(c)
    out = []
    for data, _, _ in c["operands"]:
        shp = {"a": full, "b": full, "c": full, "c_col": (full[0], 1), "c_row": (1, full[1])}[data]
        v = rng.standard_normal(shp) if data == "b" else rng.rand(*shp) + 0.5
        out.append(v.astype(c["dtype"]))
    return out


def real_reference(c, values):
    """float64 numpy, as test_fusion_gpu.expected."""
    vals = [NP_UNARY[pre[0]](v.astype(np.float64), pre[1]) for v, (_, _, pre) in zip(values, c["operands"])]
    v = vals[0]
    for u in vals[1:]:
        v = v * u if c["combine"] == "mul" else v + u
    v = NP_UNARY[c["post"][0]](c["affine"][0] * v + c["affine"][1], c["post"][1])
    full = _full(c)
    v = np.broadcast_to(v, full)
    if c["red"] is not None:
        return v.sum(axis=c["red"])
    return v[0] if len(c["shape"]) == 1 else v


def operand_kinds(c):
    """Per operand: "full", "row" (a row vector), "col" (one value per row) or "scalar", from the shape of its data."""
    o, r, col = _index_grids(c)
    full = _full(c)
    shapes = {"x7": full, "x3": full, "x7sq": full, "r3": r.shape, "r2": r.shape, "r5": r.shape, "k3": o.shape,
              "bias": col.shape, "biasr": col.shape, "a": full, "b": full, "c": full, "c_col": (full[0], 1), "c_row": (1, full[1])}
    kinds = []
    for data, _, _ in c["operands"]:
        shp = (1, 1) if isinstance(data, tuple) else tuple(shapes[data])
        kinds.append("full" if shp == tuple(full) else "scalar" if shp == (1, 1) else "row" if shp[0] == 1 else "col")
    return kinds


def request(c):
    """The request as bsc_map_reduce gets it: extents and strides (in elements) of the kept and the reduced axes."""
    ks, rs = [], []
    if len(c["shape"]) == 1:
        N = c["shape"][0]
        for kind in operand_kinds(c):
            ks.append([1 if kind == "full" else 0])
            rs.append([])
        return dict(keep_shape=[N], red_shape=[], keep_strides=ks, red_strides=rs, out_strides=[1])
    A, B = c["shape"]
    for kind, (_, pad, _) in zip(operand_kinds(c), c["operands"]):
        s = {"full": (B + pad, 1), "row": (0, 1), "col": (1, 0), "scalar": (0, 0)}[kind]
        if c["red"] is None:
            ks.append(list(s)), rs.append([])
        else:
            ks.append([s[1 - c["red"]]]), rs.append([s[c["red"]]])
    if c["red"] is None:
        return dict(keep_shape=[A, B], red_shape=[], keep_strides=ks, red_strides=rs, out_strides=[B, 1])
    return dict(keep_shape=[c["shape"][1 - c["red"]]], red_shape=[c["shape"][c["red"]]], keep_strides=ks, red_strides=rs,
                out_strides=[c["out_inner"]])


def is_linear(c):
    """linear_ops (csrc/bsc_fused.hip:955-963) for the ops these cases use."""
    return c["post"] == COPY and all(pre == COPY or pre == ("pow", -1.0) for _, _, pre in c["operands"])


def plan_for(c, options, cu):
    return fp.plan(cu=cu, linear=is_linear(c), dtype=fp.F32 if c["dtype"] == F32 else fp.F64, **dict(request(c), **options))


def check_plan(c, options, expect, cu):
    """The kernel, steps and splits the case was built for; -> the plan."""
    p = plan_for(c, options, cu)
    tag = "%s %s on %d CUs: %s" % (c["shape"], options, cu, p)
    assert p["kernel"] == expect["kernel"], tag
    for key in ("steps", "splits", "linear", "lanes_per_row", "chunks", "col_chunk", "unroll"):
        if key in expect:
            assert p[key] == expect[key], (key, tag)
    if "min_steps" in expect:
        assert p["steps"] >= expect["min_steps"], tag
    if "min_splits" in expect:
        assert p["splits"] >= expect["min_splits"], tag
    if expect.get("pstep") == "nonzero":
        assert p["pstep"], tag
    if "finish_unrolled" in expect:
        assert p["finish"] and p["finish"]["wave_per_output"] and p["finish"]["unrolled"] >= expect["finish_unrolled"], tag
    if "finish_per_thread" in expect:
        assert p["finish"] and not p["finish"]["wave_per_output"], tag
    return p


def rows_wg_for(cu):
    """rows_wg = 1 wherever two persistent steps (16 cu + 21 rows) clear short_rows' floor of 4 096 outputs
    (csrc/bsc_fused.hip:1290): 256 CUs and more.  Below that, the smallest rows_wg that does."""
    return max(1, -(-256 // cu))


def rows_cases(cu):
    """1. the short-row reduce at k = 2, 3, 5 persistent steps; rows_wg = 0 and the default context take one."""
    w = rows_wg_for(cu)
    out = collections.OrderedDict()
    variants = {
        "one-linear": dict(operands=["x7"]),
        "two-strided-linear": dict(operands=[("x7", 4, COPY), "r3"], out_inner=2),
        "three-pow-abs": dict(operands=[sq(), "r3", "k3"], post=("abs_", 0.0)),
    }
    for k, n_red in [(k, n) for k in (2, 3, 5) for n in (4, 64, 260)] + [(2, 1024)]:
        n_out = (k - 1) * 16 * cu * w + 16 + 5
        for name, kw in variants.items():
            lin = name.endswith("linear")
            runs = [({"rows_wg": w}, dict(kernel=ROWS, steps=k, splits=1, linear=lin)),
                    ({"rows_wg": 0}, dict(kernel=ROWS, steps=1, splits=1, linear=lin)),
                    ({}, dict(kernel=ROWS, steps=1, splits=1, linear=lin))]
            out["k%d-red%d-%s" % (k, n_red, name)] = case((n_out, n_red), 1, runs=runs, **kw)
    return out


def dense_map_cases(cu):
    """2. the dense map: two sweeps and 256 + 3 float4, two sweeps and 5 float4 (the second float4 in flight is wholly
    past the end)."""
    sweep = 512 * cu
    out = collections.OrderedDict()
    for tail in (256 + 3, 5):
        N = 4 * (2 * sweep + tail)
        out["five-tail%d" % tail] = case((N,), None, ["x7", "r3", "r2", "r5", ("const", 3)], runs=[
            (BLOCKS1, dict(kernel=DENSE, steps=3)), ({}, dict(kernel=DENSE, steps=1))])
        out["two-and-scalar-tail%d" % tail] = case((N,), None, ["x7", "r3", ("const", 3)], runs=[
            (dict(BLOCKS1, **NOFLAT), dict(kernel=DENSE, steps=3)), (NOFLAT, dict(kernel=DENSE, steps=1)),
            ({}, dict(kernel=FLAT, steps=1))])
    return out


def periodic_widths(cu):
    """C of the periodic cases.  A width whose period C / 4 divides the sweep of 512 cu float4 would have pstep == 0 (the
    wrap never runs): it is replaced by the next multiple of 4 above it that does not."""
    out = []
    for C in (12, 20, 36, 100, 252):
        while (512 * cu) % (C // 4) == 0 or C in out:
            C += 4
        assert C < 256
        out.append(C)
    return out


def periodic_cases(cu):
    """3. the periodic map: X dense, a bias row vector c + 1, a scalar; three sweeps, the last one ragged."""
    sweep = 512 * cu
    out = collections.OrderedDict()
    for slot, C in zip((12, 20, 36, 100, 252), periodic_widths(cu)):
        R = (2 * sweep * 4) // C + 38
        nonzero = dict(kernel=DENSE, steps=3, pstep="nonzero")
        out["three-C%d" % slot] = case((R, C), None, ["x7", "bias", ("const", 2)], runs=[
            (dict(BLOCKS1, **NOFLAT), nonzero), (NOFLAT, dict(kernel=DENSE, steps=1)), ({}, dict(kernel=FLAT, steps=1))])
        out["five-C%d" % slot] = case((R, C), None, ["x7", "bias", ("const", 2), "x3", "biasr"], runs=[
            (BLOCKS1, nonzero), ({}, dict(kernel=DENSE, steps=1))])
    return out


def row_map_cases(cu):
    """4. the row map: X with a row stride of C + 4, one value per row, a row vector."""
    ops = [("x7", 4, COPY), "k3", "bias"]
    out = collections.OrderedDict()
    for C in (64, 260, 1028):
        out["three-steps-C%d" % C] = case((2 * 8 * cu + 8 + 3, C), None, ops, runs=[
            (BLOCKS1, dict(kernel=ROWMAP, steps=3, chunks=1)), ({}, dict(kernel=ROWMAP, steps=1))])
    out["four-chunks"] = case((8, 3 * 1024 + 4), None, ops, runs=[
        (BLOCKS1, dict(kernel=ROWMAP, steps=1, chunks=4, col_chunk=1024)), ({}, dict(kernel=ROWMAP, chunks=4, col_chunk=1024))])
    out["three-chunks"] = case((5, 2052), None, ops, runs=[
        (BLOCKS1, dict(kernel=ROWMAP, steps=1, chunks=3, col_chunk=768)), ({}, dict(kernel=ROWMAP, chunks=3, col_chunk=768))])
    return out


def narrow_n_red(n_out, k):
    R = 64 // (n_out // 4)
    return 16 * R * (4 * k + 1) + R + 1


def split_cases(cu):
    """5. splits > 1, at the default context and at fused_waves_per_cu = 1."""
    out = collections.OrderedDict()

    def both(kernel, first=None, second=None, **common):
        return [({}, dict(dict(kernel=kernel, min_splits=2, **common), **(first or {}))),
                (WAVES1, dict(dict(kernel=kernel, **common), **(second or {})))]

    # a wave per (output, split), 16 bytes per lane
    out["wave-dense-1x8196"] = case((1, 8196), 1, ["x7", "r3"], both(WAVE_DENSE, unroll=4, linear=True))
    out["wave-dense-4x8196-pow-abs"] = case((4, 8196), 1, [sq(), "r3"], both(WAVE_DENSE, unroll=4, linear=False),
                                            post=("abs_", 0.0))
    out["wave-dense-7x21492"] = case((7, 21492), 1, ["x7", "r3", "k3"], both(WAVE_DENSE, unroll=4))
    out["wave-dense-8x300000"] = case((8, 300000), 1, ["x3", "r2"], both(WAVE_DENSE, unroll=4), affine=UNIT)
    out["wave-dense-1x1069060-finish-unrolled"] = case(
        (1, 4096 * 261 + 4), 1, ["x3", "r2"], both(WAVE_DENSE, first=dict(min_splits=193, finish_unrolled=1)), affine=UNIT)
    # ... scalar loads (n_red % 4 != 0)
    out["wave-3x8195"] = case((3, 8195), 1, ["x7", "r3"], both(WAVE))
    out["wave-5x20483"] = case((5, 20483), 1, ["x7", "r3", "k3"], both(WAVE))
    out["wave-3x8195-f64"] = case((3, 8195), 1, ["x7", "r3"], both(WAVE), dtype=F64)
    # lanes over outputs, 16 bytes per lane: [n_red, n_out] matrices summed over their rows
    out["lane-dense-260x133"] = case((133, 260), 0, ["x7", "r3"], both(LANE_DENSE, linear=True))
    out["lane-dense-260x453-pow-abs"] = case((453, 260), 0, [sq(), "k3"], both(LANE_DENSE, linear=False), post=("abs_", 0.0))
    out["lane-dense-1024x1000"] = case((1000, 1024), 0, ["x7", "r3", "k3"], both(LANE_DENSE))
    out["lane-dense-4096x261-finish-per-thread"] = case((261, 4096), 0, ["x7", "r3"],
                                                       both(LANE_DENSE, first=dict(finish_per_thread=True)))
    out["lane-18x193"] = case((193, 18), 0, ["x7", "r3"], both(LANE))
    out["lane-70x321"] = case((321, 70), 0, ["x7", "r3", "k3"], both(LANE))
    out["lane-4097x1030"] = case((1030, 4097), 0, ["x7", "r3"], both(LANE, first=dict(finish_per_thread=True)))
    out["lane-18x193-f64"] = case((193, 18), 0, ["x7", "r3"], both(LANE), dtype=F64)
    # fewer than 256 outputs: L = n_out / 4 lanes per row, 64 / L rows per wave load
    for n_out in (16, 20, 28, 36, 64, 100, 124, 128):
        for k in (1, 3):
            plan = dict(kernel=NARROW, lanes_per_row=n_out // 4, splits=k, steps=6 if k == 1 else 5)
            for name, ops in (("kept-rider", ["x7", "k3"]), ("row-value", ["x7", "r3"])):
                out["narrow-%d-splits%d-%s" % (n_out, k, name)] = case(
                    (narrow_n_red(n_out, k), n_out), 0, ops, runs=[({}, plan), (WAVES1, plan)])
    return out


PRE_REAL = [("log", 0.0), ("exp", 0.0), ("pow", -1.0)]


def parity_cases(cu):
    """6. one case per kernel from the lists above on real values.  -> {name: (kernel, case)}; the combine is set by the
    test."""
    sweep, w = 512 * cu, rows_wg_for(cu)

    def real(shape, red, third, runs, pads=(0, 0), dtype=F32, seed=0):
        ops = [("a", pads[0], PRE_REAL[0]), ("b", pads[1], PRE_REAL[1]), (third, 0, PRE_REAL[2])]
        return case(shape, red, ops, runs, affine=HALF, post=("abs_", 0.0), dtype=dtype, seed=seed)

    multi = dict(min_splits=2)
    out = collections.OrderedDict()
    out["rows"] = real((16 * cu * w + 21, 260), 1, "c_col", [({"rows_wg": w}, dict(kernel=ROWS, steps=2, linear=False))], seed=1)
    out["dense-map"] = real((4 * (2 * sweep + 259),), None, "c", [(dict(BLOCKS1, **NOFLAT), dict(kernel=DENSE, steps=3))], seed=2)
    out["periodic-map"] = real(((2 * sweep * 4) // periodic_widths(cu)[3] + 38, periodic_widths(cu)[3]), None, "c_row",
                               [(dict(BLOCKS1, **NOFLAT), dict(kernel=DENSE, steps=3, pstep="nonzero"))], seed=3)
    out["row-map"] = real((2 * 8 * cu + 11, 260), None, "c_col", [(BLOCKS1, dict(kernel=ROWMAP, steps=3))], pads=(4, 4), seed=4)
    out["wave-dense"] = real((8, 300000), 1, "c_col", [({}, dict(kernel=WAVE_DENSE, **multi))], seed=5)
    out["wave"] = real((5, 20483), 1, "c_col", [({}, dict(kernel=WAVE, **multi))], seed=6)
    out["wave-f64"] = real((5, 20483), 1, "c_col", [({}, dict(kernel=WAVE, **multi))], dtype=F64, seed=7)
    out["lane-dense"] = real((453, 260), 0, "c_col", [({}, dict(kernel=LANE_DENSE, **multi))], seed=8)
    out["lane"] = real((321, 70), 0, "c_col", [({}, dict(kernel=LANE, **multi))], seed=9)
    out["lane-f64"] = real((321, 70), 0, "c_col", [({}, dict(kernel=LANE, **multi))], dtype=F64, seed=10)
    out["narrow"] = real((narrow_n_red(100, 3), 100), 0, "c_col", [({}, dict(kernel=NARROW, splits=3, lanes_per_row=25))], seed=11)
    return out


EXACT_TABLES = collections.OrderedDict([("rows", rows_cases), ("dense_map", dense_map_cases), ("periodic", periodic_cases),
                                        ("row_map", row_map_cases), ("splits", split_cases)])
REDUCE_PARITY = ("rows", "wave-dense", "wave", "lane-dense", "lane", "narrow")       # 7. one case per reduce kernel


# ---- the device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cu(ctx):
    n = int(ctx.info()["cu_count"])
    print("cu_count %d" % n)
    return n


@pytest.fixture(scope="module")
def alt(ctx):
    """alt(name=value) -> a second Context on the session context's device and stream (tests/test_view_routes_gpu.py's);
    alt() is the session context itself."""
    from bayesic_amd.device import Context
    made = {}

    def get(**options):
        if not options:
            return ctx
        key = tuple(sorted(options.items()))
        if key not in made:
            made[key] = Context(ctx.device_index, stream=ctx.stream, options=options)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _i64(v):
    v = list(v)
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def upload(c, values, dev):
    """The operands as views of NaN-padded buffers, in the layout `request` describes."""
    views = []
    for v, kind, (_, pad, _) in zip(values, operand_kinds(c), c["operands"]):
        v = np.asarray(v, c["dtype"])
        if kind == "full" and len(c["shape"]) == 2:
            views.append(V.place(v, V.Layout(ld_extra=pad), dev))
        else:
            views.append(V.place(v.reshape(-1), V.DENSE, dev))
    return views


def launch(cx, c, views):
    """One bsc_map_reduce call (the C ABI, as tests/test_fusion_gpu.py's map_reduce) into a fresh guarded output;
    -> the result on the host, after the guard check."""
    q = request(c)
    dev = views[0].buf.device
    if c["red"] is None:
        out = V.out_like(c["shape"], c["dtype"], V.DENSE, dev)
    else:
        out = V.out_like((q["keep_shape"][0],), c["dtype"], V.Layout(inner=c["out_inner"]), dev)
    assert list(out.strides) == q["out_strides"] and all(V.misalignment(v) == 0 for v in views + [out])
    n = len(views)
    cx.call("bsc_map_reduce", 0 if c["dtype"] == F32 else 1, OPS[c["combine"]], len(q["keep_shape"]), _i64(q["keep_shape"]),
            len(q["red_shape"]), _i64(q["red_shape"]), n, (ctypes.c_void_p * n)(*[v.ptr for v in views]),
            _i64(s for row in q["keep_strides"] for s in row), _i64(s for row in q["red_strides"] for s in row),
            (ctypes.c_int32 * n)(*[OPS[pre[0]] for _, _, pre in c["operands"]]),
            (ctypes.c_double * n)(*[float(pre[1]) for _, _, pre in c["operands"]]), float(c["affine"][0]), float(c["affine"][1]),
            OPS[c["post"][0]], float(c["post"][1]), out.ptr, _i64(q["out_strides"]))
    cx.sync()
    got = out.numpy()
    out.check_guard()
    return got


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def assert_bits(got, want, tag):
    bad = np.flatnonzero(_bits(got).reshape(-1) != _bits(np.asarray(want, got.dtype)).reshape(-1))
    if bad.size:
        g, w = got.reshape(-1).astype(np.float64), np.asarray(want, np.float64).reshape(-1)
        raise AssertionError("%s: %d of %d outputs differ; the first at flat index %d: got %r, want %r; largest difference %r"
                             % (tag, bad.size, g.size, bad[0], g[bad[0]], w[bad[0]], np.nanmax(np.abs(g[bad] - w[bad]))))


def run_exact(ctx, alt, cu, c, name):
    want = exact_reference(c)
    assert (want.astype(c["dtype"]).astype(np.float64) == want).all()
    views = upload(c, [stored for stored, _ in exact_values(c)], ctx.device)
    if c["red"] is None and is_linear(c):         # a map of linear ops: the same arithmetic in numpy float32, in the kernel's order
        f32 = np.ones(want.shape, F32)
        for stored, _ in exact_values(c):
            f32 = f32 * (stored.astype(F32)[0] if len(c["shape"]) == 1 else stored.astype(F32))
        assert_bits(f32 * F32(c["affine"][0]) + F32(c["affine"][1]), want, name + ": numpy float32")
    first = None
    for options, expect in c["runs"]:
        p = check_plan(c, options, expect, cu)
        got = launch(alt(**options), c, views)
        assert got.shape == want.shape and got.dtype == c["dtype"]
        assert_bits(got, want, "%s %s (%s, steps %d, splits %d)" % (name, options, p["kernel"], p["steps"], p["splits"]))
        if first is None:
            first = got
        assert_bits(got, first, "%s %s against the first context" % (name, options))


# ---- 1-5. exact accounting -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rows_cases(256)))
def test_short_row_reduce_takes_several_persistent_steps(ctx, alt, cu, name):
    run_exact(ctx, alt, cu, rows_cases(cu)[name], name)


@pytest.mark.parametrize("name", list(dense_map_cases(256)))
def test_dense_map_takes_three_sweeps(ctx, alt, cu, name):
    run_exact(ctx, alt, cu, dense_map_cases(cu)[name], name)


@pytest.mark.parametrize("name", list(periodic_cases(256)))
def test_periodic_map_wraps_its_row_vector_index(ctx, alt, cu, name):
    run_exact(ctx, alt, cu, periodic_cases(cu)[name], name)


@pytest.mark.parametrize("name", list(row_map_cases(256)))
def test_row_map_takes_three_row_steps_and_column_chunks(ctx, alt, cu, name):
    run_exact(ctx, alt, cu, row_map_cases(cu)[name], name)


@pytest.mark.parametrize("name", list(split_cases(256)))
def test_split_reductions(ctx, alt, cu, name):
    run_exact(ctx, alt, cu, split_cases(cu)[name], name)


# ---- 6, 7. parity on real values; determinism -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _parity(cu, name, combine):
    c = dict(parity_cases(cu)[name], combine=combine)
    values = real_values(c)
    want = real_reference(c, values)
    want.setflags(write=False)
    return c, values, want


@pytest.mark.parametrize("combine", ["mul", "add"])
@pytest.mark.parametrize("name", list(parity_cases(256)))
def test_parity_on_real_values(ctx, alt, cu, name, combine):
    c, values, want = _parity(cu, name, combine)
    (options, expect), = c["runs"]
    p = check_plan(c, options, expect, cu)
    got = launch(alt(**options), c, upload(c, values, ctx.device))
    tol = 1e-5 if c["dtype"] == F32 else 1e-12
    err = np.abs(got.astype(np.float64) - want)
    bound = tol + tol * np.abs(want)
    print("%s %s (%s, steps %d, splits %d): worst err / bound %.3g" % (name, combine, p["kernel"], p["steps"], p["splits"],
                                                                       float((err / bound).max())))
    assert got.shape == want.shape and (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("name", REDUCE_PARITY)
def test_two_runs_are_bit_identical(ctx, alt, cu, name):
    c, values, _ = _parity(cu, name, "mul")
    (options, expect), = c["runs"]
    check_plan(c, options, expect, cu)
    views = upload(c, values, ctx.device)
    one, two = launch(alt(**options), c, views), launch(alt(**options), c, views)
    assert_bits(two, one, name)
