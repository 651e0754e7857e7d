"""tests/_fused_plan.py (the dispatcher of csrc/bsc_fused.hip restated) and the case tables of
tests/test_fused_multi_step_gpu.py, without a device: the tables land on the kernel, split count and step count each
case is named for at 64, 256 and 304 CUs, every exact-accounting reference is exactly representable in the output's
type, and the plan agrees with values worked out by hand from the C++ at 256 CUs."""
import numpy as np
import pytest

import _fused_plan as fp
import test_fused_multi_step_gpu as ms

CUS = (256, 64, 304)


def _reduce(n_out, n_red, lanes, n_in=1, **ctx):
    """sum over n_red of a dense matrix: [n_out, n_red] (a wave per output) or [n_red, n_out] (lanes over outputs)."""
    ks, rs = ([1], [n_out]) if lanes else ([n_red], [1])
    return fp.plan([n_out], [n_red], [ks] * n_in, [rs] * n_in, [1], **ctx)


# ---- the restatement ------------------------------------------------------------------------------------------------

def test_dense_matrix_coalesces_to_rank_one_and_a_row_vector_stops_it():
    R, C = 1000, 64
    dense, scalar, rowvec, percol = [C, 1], [0, 0], [0, 1], [1, 0]
    keep, red, ks, rs, outs = fp.normalise([R, C], [], [dense, dense, scalar], [[], [], []], [C, 1])
    assert keep == [R * C] and red == [] and ks == [[1], [1], [0]] and outs == [1]
    keep, _, ks, _, outs = fp.normalise([R, C], [], [dense, rowvec], [[], []], [C, 1])
    assert keep == [R, C] and ks == [[C, 1], [0, 1]] and outs == [C, 1]
    keep, _, ks, _, _ = fp.normalise([R, C], [], [dense, percol], [[], []], [C, 1])
    assert keep == [R, C] and ks == [[C, 1], [1, 0]]
    # a padded row stride does not merge either; extent-1 axes go
    assert fp.normalise([R, C], [], [[C + 4, 1]], [[]], [C, 1])[0] == [R, C]
    assert fp.normalise([1, R, 1, C], [], [[7, C, 9, 1]], [[]], [0, C, 0, 1])[0] == [R * C]


def test_axes_are_sorted_by_the_output_and_by_the_widest_operand():
    # a transposed output view: the kept axes are walked in the output's order and coalesce like the original
    keep, _, ks, _, outs = fp.normalise([5, 7], [], [[1, 5]], [[]], [1, 5])
    assert keep == [35] and ks == [[1]] and outs == [1]
    # two reduced axes around a kept one ((20, 30, 40) summed over 0 and 2): the big operand orders them
    keep, red, ks, rs, _ = fp.normalise([30], [40, 20], [[40], [0]], [[1, 1200], [0, 1]], [1])
    assert red == [20, 40] and rs == [[1200, 1], [1, 0]]
    assert fp.normalise([0, 3], [4], [[3, 1]], [[0]], [3, 1]) is None


@pytest.mark.parametrize("stride", [4, 64])
def test_unrolled_loop_trip_counts_against_the_loops_themselves(stride):
    for length in list(range(0, 40 * stride, 7)) + [3 * stride, 3 * stride + 1, 4 * stride, 7 * stride, 7 * stride + 1]:
        r = first = tail = 0
        while r + 3 * stride < length:
            r, first = r + 4 * stride, first + 1
        while r < length:
            r, tail = r + stride, tail + 1
        assert fp._unrolled_trips(length, stride) == (first, tail), length


def test_spot_values_checked_by_hand_at_256_cus():
    w1 = dict(fused_waves_per_cu=1)
    for n_out, n_red, lanes, ctx, kernel, splits in [
            (8, 300000, False, {}, ms.WAVE_DENSE, 73),                       # 1024 * 4 / 8 = 512, at most 300000 / 4096
            (8, 300000, False, w1, ms.WAVE_DENSE, 32),                       # 64 * 4 / 8
            (1, 4096 * 261 + 4, False, {}, ms.WAVE_DENSE, 261),
            (4097, 1030, True, {}, ms.LANE, 15),                             # 65 jobs: 1024 / 65, at most 1030 / 64 = 16
            (4097, 1030, True, w1, ms.LANE, 1),                              # 65 jobs >= 64 blocks wanted
            (4096, 261, True, {}, ms.LANE_DENSE, 4),                         # 261 / 64
            (20, 2509, True, {}, ms.NARROW, 3)]:                             # L = 5, R = 12: 2509 / (16 * 12 * 4)
        p = _reduce(n_out, n_red, lanes, cu=256, **ctx)
        assert (p["kernel"], p["splits"]) == (kernel, splits), (n_out, n_red, ctx, p)
    p = _reduce(20, 2509, True, cu=256)
    assert p["lanes_per_row"] == 5 and p["grid"] == (3, 1) and p["steps"] == 5          # 14 steps of 192 rows over 3 splits
    p = _reduce(1, 4096 * 261 + 4, False, cu=256)
    assert p["keep"] == [] and p["finish"] == dict(wave_per_output=True, grid=1, unrolled=1, steps=2)
    p = _reduce(4096, 261, True, cu=256)
    assert p["finish"] == dict(wave_per_output=False, grid=16, unrolled=0, steps=4) and p["grid"] == (64, 1)


def test_step_thresholds_at_the_default_options():
    """The thresholds the suite never crossed: 64 * 256 * 16 rows, 1 M float4, 16 384 rows of a row map."""
    rows = lambda n: _reduce(n, 64, False, n_in=2, cu=256)
    assert rows(262144)["kernel"] == ms.ROWS and rows(262144)["steps"] == 1 and rows(262145)["steps"] == 2
    assert rows(4095)["kernel"] == ms.WAVE_DENSE and rows(4096)["kernel"] == ms.ROWS
    assert _reduce(4096, 1028, False, cu=256)["kernel"] == ms.WAVE_DENSE
    assert _reduce(4096, 64, False, cu=256, fused_map_flat=0)["kernel"] == ms.WAVE_DENSE
    dense = lambda n4: fp.plan([4 * n4], [], [[1]] * 5, [[]] * 5, [1], cu=256)
    assert dense(1 << 20)["kernel"] == ms.DENSE and dense(1 << 20)["steps"] == 1 and dense((1 << 20) + 1)["steps"] == 2
    rowmap = lambda R: fp.plan([R, 64], [], [[68, 1], [1, 0]], [[], []], [64, 1], cu=256)
    assert rowmap(16384)["kernel"] == ms.ROWMAP and rowmap(16384)["steps"] == 1 and rowmap(16385)["steps"] == 2
    # the one two-sweep periodic case the suite had, (100 003, 64) with five operands: the wrap never runs
    old = fp.plan([100003, 64], [], [[64, 1]] * 2 + [[0, 1]] * 3, [[]] * 5, [64, 1], cu=256)
    assert old["kernel"] == ms.DENSE and old["steps"] == 2 and old["pstep"] == 0


def test_routes_the_cases_must_not_take():
    flat = fp.plan([1000, 64], [], [[64, 1], [0, 1]], [[], []], [64, 1], cu=256)
    assert flat["kernel"] == ms.FLAT and flat["grid"] == (16, 1)
    assert fp.plan([1000, 64], [], [[64, 1], [0, 1]], [[], []], [64, 1], align=[4, 0, 0], cu=256)["kernel"] == "map_small_f32_kernel"
    assert fp.plan([37, 53], [], [[53, 1]], [[]], [53, 1], cu=256)["kernel"] == "map_small_f32_kernel"
    assert fp.plan([37, 53], [], [[53, 1]], [[]], [53, 1], dtype=fp.F64, cu=256)["kernel"] == "map_strided_kernel"
    # misaligned or float64 reductions: the generic kernels
    assert fp.plan([64], [4096], [[4096]], [[1]], [1], align=[8, 0], cu=256)["kernel"] == ms.WAVE
    assert fp.plan([64], [4096], [[4096]], [[1]], [1], dtype=fp.F64, cu=256)["kernel"] == ms.WAVE
    assert fp.plan([96], [4096], [[1]], [[96]], [1], special=True, cu=256)["kernel"] == ms.LANE
    # fewer than 16 outputs: a wave per output even when the kept axis is the fast one
    assert fp.plan([8], [300000], [[1]], [[8]], [1], cu=256)["kernel"] == ms.WAVE


# ---- the tables -------------------------------------------------------------------------------------------------------

TABLES = dict(ms.EXACT_TABLES, parity=ms.parity_cases)


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("table", list(TABLES))
def test_every_case_lands_on_what_it_is_named_for(table, cu):
    cases = TABLES[table](cu)
    assert list(cases) == list(TABLES[table](256))                 # the ids the GPU module is parametrised with
    for name, c in cases.items():
        assert c["runs"], name
        for options, expect in c["runs"]:
            ms.check_plan(c, options, expect, cu)
        assert (c["seed"] is None) == (table != "parity")


@pytest.mark.parametrize("cu", CUS)
def test_the_tables_reach_what_the_issue_lists(cu):
    rows = ms.rows_cases(cu)
    w = ms.rows_wg_for(cu)
    assert (w == 1) == (cu >= 256)
    assert sorted({c["shape"][0] for c in rows.values()}) == [(k - 1) * 16 * cu * w + 21 for k in (2, 3, 5)]
    if cu == 256:
        assert sorted({c["shape"][0] for c in rows.values()}) == [4117, 8213, 16405]
        assert sorted({c["shape"][0] for n, c in ms.row_map_cases(cu).items() if "steps" in n}) == [4107]
        assert ms.periodic_widths(cu) == [12, 20, 36, 100, 252]
    assert sorted({c["shape"][1] for c in rows.values()}) == [4, 64, 260, 1024]
    assert {len(c["operands"]) for c in rows.values()} == {1, 2, 3}
    assert {c["out_inner"] for c in rows.values()} == {1, 2} and {p for c in rows.values() for _, p, _ in c["operands"]} == {0, 4}
    assert {ms.is_linear(c) for c in rows.values()} == {True, False}
    for name, c in ms.periodic_cases(cu).items():
        assert ms.plan_for(c, c["runs"][0][0], cu)["pstep"] != 0, name
    narrow = {n: c for n, c in ms.split_cases(cu).items() if n.startswith("narrow")}
    assert sorted({c["shape"][1] for c in narrow.values()}) == [16, 20, 28, 36, 64, 100, 124, 128]
    for c in narrow.values():
        n_red, n_out = c["shape"]
        R = 64 // (n_out // 4)
        assert n_red % (16 * R) == R + 1                           # a ragged last step of R + 1 rows
    # every reduce kernel sees splits > 1 in some case, and the finish kernel both of its forms
    seen = {}
    for c in ms.split_cases(cu).values():
        p = ms.plan_for(c, {}, cu)
        seen.setdefault(p["kernel"], []).append(p)
    assert set(seen) == {ms.WAVE_DENSE, ms.WAVE, ms.LANE_DENSE, ms.LANE, ms.NARROW}
    assert all(max(p["splits"] for p in ps) > 1 for ps in seen.values())
    assert any(p["finish"] and p["finish"]["unrolled"] for p in seen[ms.WAVE_DENSE])
    assert any(p["finish"] and not p["finish"]["wave_per_output"] for p in seen[ms.LANE_DENSE])


@pytest.mark.parametrize("table", list(ms.EXACT_TABLES))
def test_exact_references_are_exact_in_the_output_type(table):
    """An integer below 2^24 or a multiple of 1/4 below 2^22: float32(ref) == ref, for every output of every case."""
    for name, c in ms.EXACT_TABLES[table](256).items():
        ref = ms.exact_reference(c)
        want_shape = c["shape"] if c["red"] is None else (c["shape"][1 - c["red"]],)
        assert ref.shape == tuple(want_shape) and ref.dtype == np.float64, name
        assert (ref * 4 == np.round(ref * 4)).all() and ref.min() >= 0.75, name
        whole = (ref == np.round(ref)).all()
        assert ref.max() < (2 ** 24 if whole else 2 ** 22), (name, ref.max())
        assert (ref.astype(np.float32).astype(np.float64) == ref).all(), name
        # ... and every per-element value before the sum (products of at most five small integers)
        for stored, eff in ms.exact_values(c):
            assert 1 <= stored.min() and stored.max() < 2 ** 24 and 1 <= eff.min()
