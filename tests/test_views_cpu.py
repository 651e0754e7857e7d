"""The view harness (tests/_views.py) proved on the CPU, and the coverage of the case tables of
tests/test_view_routes_gpu.py.

The harness is only worth something if a subtly wrong kernel fails it.  Here numpy "kernels" that are wrong
on purpose -- each in one of the ways an alignment-gated GPU kernel goes wrong -- run over torch CPU tensors
laid out by the harness; each must fail the value check or the guard check, and the correct one must pass
every layout.  No GPU kernel is broken to show this."""
import numpy as np
import pytest
import torch

import _views as V
from _views import Layout

LAYOUTS = [Layout(), Layout(base_off=1), Layout(base_off=3, ld_extra=1), Layout(ld_extra=5), Layout(base_off=2, ld_extra=4),
           Layout(ld_extra=3, inner=2), Layout(base_off=1, transpose=True, ld_extra=2)]


# ---- fake kernels: out[r, c] = 2 in[r, c] + 1 on flat buffers, told (offset, row stride, element stride) -----------
def k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    for r in range(rows):
        for c in range(cols):
            dst[do + r * d_r + c * d_c] = 2 * src[so + r * s_r + c * s_c] + 1


def k_ignores_input_base(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    """Rounds the input pointer down to 16 bytes, as an unguarded 16-byte load does."""
    k_correct(src, so & ~3, s_r, s_c, dst, do, d_r, d_c, rows, cols)


def k_ignores_output_base(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    k_correct(src, so, s_r, s_c, dst, do & ~3, d_r, d_c, rows, cols)


def k_dense_input_ld(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    """Takes the packed leading dimension instead of the one it was given."""
    s_r, s_c = (cols * s_c, s_c) if s_r >= s_c else (s_r, rows * s_r)
    k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols)


def k_dense_output_ld(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    d_r, d_c = (cols * d_c, d_c) if d_r >= d_c else (d_r, rows * d_r)
    k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols)


def k_wide_store_at_row_end(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    """Stores whole groups of four along the contiguous output axis: three elements too many at a ragged end."""
    k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols)
    n_out, n_in, st_out, st_in = (rows, cols, d_r, d_c) if d_r >= d_c else (cols, rows, d_c, d_r)
    for o in range(n_out):
        last = do + o * st_out + (n_in - 1) * st_in
        for extra in (1, 2, 3):
            dst[last + extra * st_in] = dst[last]


def k_writes_one_before(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
    k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols)
    dst[do - 1] = 0.0


def run(kernel, a, lay_in, lay_out):
    """-> (values ok, guard ok): the order of checks the GPU tests use."""
    src = V.place(a, lay_in)
    dst = V.out_like(a.shape, a.dtype, lay_out)
    kernel(src.buf.numpy(), src.offset, src.strides[0], src.strides[1],
           dst.buf.numpy(), dst.offset, dst.strides[0], dst.strides[1], *a.shape)
    got = dst.numpy()
    values = bool(np.array_equal(got, 2 * a + 1))          # NaN (poison, or an unwritten sentinel) is never equal
    guard = dst.touched().size == 0
    return values, guard


def data(rows=7, cols=10, dtype=np.float32):
    return np.random.RandomState(rows * 31 + cols).standard_normal((rows, cols)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("lay_out", LAYOUTS, ids=Layout.describe)
@pytest.mark.parametrize("lay_in", LAYOUTS, ids=Layout.describe)
def test_a_correct_kernel_passes_every_layout(lay_in, lay_out, dtype):
    assert run(k_correct, data(dtype=dtype), lay_in, lay_out) == (True, True)


@pytest.mark.parametrize("off", [1, 2, 3])
def test_ignoring_the_input_base_offset_is_caught_by_the_values(off):
    values, guard = run(k_ignores_input_base, data(), Layout(base_off=off), Layout())
    assert not values and guard


@pytest.mark.parametrize("off", [1, 2, 3])
def test_ignoring_the_output_base_offset_is_caught_by_the_guard_and_the_values(off):
    out = V.out_like((7, 10), np.float32, Layout(base_off=off, ld_extra=1))
    values, guard = run(k_ignores_output_base, data(), Layout(), Layout(base_off=off, ld_extra=1))
    assert not values and not guard
    # ... and the report names the first touched element: `off` before the view
    a = data()
    src, dst = V.place(a), out
    k_ignores_output_base(src.buf.numpy(), src.offset, *src.strides, dst.buf.numpy(), dst.offset, *dst.strides, *a.shape)
    with pytest.raises(AssertionError, match=r"offset -%d from" % off):
        dst.check_guard()


@pytest.mark.parametrize("extra", [1, 2, 3, 4, 5])
def test_the_dense_leading_dimension_on_the_input_is_caught_by_the_values(extra):
    values, guard = run(k_dense_input_ld, data(), Layout(ld_extra=extra), Layout())
    assert not values and guard
    values, guard = run(k_dense_input_ld, data(), Layout(ld_extra=extra, transpose=True), Layout())
    assert not values and guard


@pytest.mark.parametrize("extra", [1, 2, 3, 4, 5])
def test_the_dense_leading_dimension_on_the_output_is_caught(extra):
    values, guard = run(k_dense_output_ld, data(), Layout(), Layout(ld_extra=extra))
    assert not values                                # rows land in the wrong place: sentinels stay where rows were due
    assert not guard                                 # ... and the row gaps are guard


@pytest.mark.parametrize("lay_out", [Layout(), Layout(ld_extra=1), Layout(ld_extra=4), Layout(base_off=2, ld_extra=5),
                                     Layout(transpose=True, ld_extra=3)], ids=Layout.describe)
def test_four_elements_stored_where_one_was_due_is_caught_by_the_guard(lay_out):
    values, guard = run(k_wide_store_at_row_end, data(7, 10), Layout(), lay_out)
    assert not guard
    if lay_out.ld_extra >= 3:
        assert values           # the overrun stayed inside the row gap: ONLY the guard sees it


def test_an_overrun_into_the_next_row_is_caught_by_the_values_when_rows_are_packed():
    values, guard = run(k_wide_store_at_row_end, data(7, 10), Layout(), Layout())
    assert not values and not guard                  # the next row's head is clobbered; the last row runs into the guard


@pytest.mark.parametrize("lay_out", LAYOUTS, ids=Layout.describe)
def test_one_element_written_before_the_view_is_caught_by_the_guard(lay_out):
    values, guard = run(k_writes_one_before, data(), Layout(), lay_out)
    assert values and not guard
    dst = V.out_like((3, 4), np.float32, lay_out)
    dst.buf[dst.offset - 1] = 0.0
    with pytest.raises(AssertionError, match=r"offset -1 from"):
        dst.check_guard()


def test_an_unwritten_output_element_is_caught_by_the_values():
    def k_skips_last(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols):
        k_correct(src, so, s_r, s_c, dst, do, d_r, d_c, rows, cols - 1)
    values, guard = run(k_skips_last, data(), Layout(), Layout(ld_extra=2))
    assert not values and guard


def test_a_write_of_the_same_value_with_other_bits_is_caught():
    """The guard is compared on integer views: another NaN, or -0.0 over 0.0, is a touch."""
    dst = V.out_like((4, 4), np.float32, Layout(ld_extra=1))
    dst.check_guard()
    dst.buf[dst.offset + 4] = float("nan")           # the gap after row 0: a NaN, but not the sentinel's bits
    assert list(dst.touched()) == [4]
    d64 = V.out_like((5,), np.float64, Layout(base_off=1))
    d64.buf[-1] = float("nan")
    assert list(d64.touched()) == [d64.buf.numel() - 1 - d64.offset]


# ---- the geometry itself ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", LAYOUTS + [Layout(batch_rem=1), Layout(base_off=2, batch_rem=3, ld_extra=1, transpose=True)],
                         ids=Layout.describe)
@pytest.mark.parametrize("shape", [(5,), (0,), (1,), (3, 6), (1, 9), (2, 3, 5)])
def test_geometry_alignment_guard_and_round_trip(lay, shape):
    a = np.arange(1, 1 + int(np.prod(shape)), dtype=np.float32).reshape(shape)
    v = V.place(a, lay)
    assert np.array_equal(v.numpy(), a)
    assert V.misalignment(v) == lay.base_off
    off, strides, length = lay.geometry(shape)
    assert tuple(v.t.stride()) == tuple(strides) and v.t.storage_offset() == off >= V.GUARD
    if a.size:
        last = off + sum((n - 1) * s for n, s in zip(shape, strides))
        assert length - 1 - last >= V.GUARD
        inside = np.zeros(length, bool)
        inside[np.unique(np.asarray(torch.as_strided(torch.arange(length), shape, strides, off)).ravel())] = True
        assert inside.sum() == a.size                           # no two elements share a slot
        assert np.isnan(v.buf.numpy()[~inside]).all()           # an input is NaN everywhere else
    if len(shape) >= 2:
        assert min(strides[-2:]) == lay.inner
        assert (strides[-1] == lay.inner) != lay.transpose
        if len(shape) == 3:
            assert strides[0] % 4 == lay.batch_rem
    o = V.out_like(shape, np.float32, lay)
    assert (o.buf.view(torch.int32).numpy().view(np.uint32) == V.SENTINEL[np.dtype(np.float32)]).all()
    o.check_guard()
    assert V.call_args(o) == (o.ptr,) + tuple(strides)
    assert not a.size or o.ptr == o.t.data_ptr()


def test_describe_is_unique_per_layout():
    seen = {}
    for b in range(4):
        for e in range(6):
            for t in (False, True):
                for i in (1, 2):
                    for r in range(4):
                        d = Layout(b, e, t, i, r).describe()
                        assert d not in seen
                        seen[d] = 1
    assert Layout().describe() == "dense" and Layout(1, 5, True, 2, 3).describe() == "off1-ld+5-T-inner2-bat+3"


# ---- the case tables of tests/test_view_routes_gpu.py --------------------------------------------------------------
def test_every_listed_axis_value_is_visited_and_every_entry_point_has_a_dense_control():
    import test_view_routes_gpu as R
    assert set(R.REQUIRED) == set(R.TABLES)
    for entry, axes in R.REQUIRED.items():
        cases = R.TABLES[entry]
        assert len(cases) and len({R.case_id(c) for c in cases}) == len(cases), entry
        seen = [R.axes_of(entry, c) for c in cases]
        for axis, values in axes.items():
            visited = set()
            for s in seen:
                v = s[axis]
                visited |= set(v) if isinstance(v, (set, frozenset)) else {v}
            missing = set(values) - visited
            assert not missing, "%s: axis %s never takes %s" % (entry, axis, sorted(missing, key=repr))
        assert any(s["control"] for s in seen), "%s has no all-dense, all-aligned case" % entry


def test_no_case_of_the_view_routes_is_skipped_or_expected_to_fail():
    import inspect
    import test_view_routes_gpu as R
    src = inspect.getsource(R)
    for word in ("pytest.skip", "xfail", "skipif", "importorskip"):
        assert word not in src, word


def test_every_reference_of_the_view_routes_is_finite():
    import test_view_routes_gpu as R
    for entry, cases in R.TABLES.items():
        for c in cases:
            for name, want in R.reference(entry, c).items():
                assert np.isfinite(np.asarray(want, np.float64)).all(), (entry, R.case_id(c), name)
