"""Operands as views of wider buffers, for the kernels that pick a route from address arithmetic.

``Layout`` says where an array lies in its buffer: the first element ``base_off`` elements past a
16-byte boundary, rows ``ld_extra`` elements further apart than they need be, optionally stored
transposed, optionally with every second element used (inner stride 2), batches a multiple of four
plus ``batch_rem`` elements apart.  ``place`` builds the buffer and returns a ``View``:

  * an INPUT buffer is NaN everywhere outside the view, so a read outside it poisons the result;
  * an OUTPUT buffer holds one fixed bit pattern (a NaN with a payload) everywhere -- inside the view
    too, so an element the kernel never writes fails the value check -- and ``View.check_guard()``
    afterwards compares every element outside the view BITWISE with that pattern and names the first
    touched offset.  At least ``GUARD`` elements of it lie before the first and after the last
    element of the view; the gaps between rows (and between the elements of an inner-stride-2 row)
    are guard as well.

The buffers are torch tensors on any device: the CPU stands in for the GPU in tests/test_views_cpu.py,
which feeds the harness kernels that are wrong on purpose.
"""
import numpy as np
import torch

GUARD = 64                                   # elements; a multiple of 4, so it keeps the base's 16-byte phase
SENTINEL = {np.dtype(np.float32): np.uint32(0x7FC5A5A5), np.dtype(np.float64): np.uint64(0x7FF85A5AA5A55A5A)}
_BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
_SIGNED = {np.dtype(np.float32): torch.int32, np.dtype(np.float64): torch.int64}


class Layout(object):
    def __init__(self, base_off=0, ld_extra=0, transpose=False, inner=1, batch_rem=0):
        assert base_off in (0, 1, 2, 3) and ld_extra in (0, 1, 2, 3, 4, 5) and inner in (1, 2) \
            and batch_rem in (0, 1, 2, 3)
        self.base_off, self.ld_extra, self.transpose, self.inner, self.batch_rem = \
            base_off, ld_extra, bool(transpose), inner, batch_rem

    @property
    def dense(self):
        """Aligned, packed, unit inner stride, not transposed: what a fresh contiguous upload is."""
        return (self.base_off, self.ld_extra, self.transpose, self.inner, self.batch_rem) == (0, 0, False, 1, 0)

    def describe(self):
        if self.dense:
            return "dense"
        parts = []
        if self.base_off:
            parts.append("off%d" % self.base_off)
        if self.ld_extra:
            parts.append("ld+%d" % self.ld_extra)
        if self.transpose:
            parts.append("T")
        if self.inner != 1:
            parts.append("inner%d" % self.inner)
        if self.batch_rem:
            parts.append("bat+%d" % self.batch_rem)
        return "-".join(parts)

    __repr__ = describe

    def geometry(self, shape):
        """(offset of the first element in the buffer, strides of the LOGICAL axes, buffer length), in
        elements.  shape is (n,), (rows, cols) or (batch, rows, cols); with ``transpose`` the last two
        axes are stored the other way round (the logical row stride is then the inner one)."""
        shape = tuple(int(s) for s in shape)
        assert 1 <= len(shape) <= 3
        offset = GUARD + self.base_off
        if len(shape) == 1:
            strides = (self.inner,)
            span = (shape[0] - 1) * self.inner + 1 if shape[0] else 0
            return offset, strides, offset + span + GUARD
        rows, cols = shape[-2:]
        s_rows, s_cols = (cols, rows) if self.transpose else (rows, cols)      # as stored
        ld = max(s_cols, 1) * self.inner + self.ld_extra
        rc = (self.inner, ld) if self.transpose else (ld, self.inner)
        if len(shape) == 2:
            strides = rc
            span = ((s_rows - 1) * ld + (s_cols - 1) * self.inner + 1) if rows and cols else 0
            return offset, strides, offset + span + GUARD
        sb = -(-(s_rows * ld) // 4) * 4 + self.batch_rem
        strides = (sb,) + rc
        span = ((shape[0] - 1) * sb + (s_rows - 1) * ld + (s_cols - 1) * self.inner + 1) \
            if shape[0] and rows and cols else 0
        return offset, strides, offset + span + GUARD


DENSE = Layout()


def _strided(host, offset, shape, strides):
    item = host.itemsize
    return np.lib.stride_tricks.as_strided(host[offset:], shape, tuple(s * item for s in strides))


class View(object):
    """``t``: the strided tensor (its data_ptr() is the operand's pointer); ``strides``: in elements, per
    logical axis; ``buf``: the flat buffer it lies in."""

    def __init__(self, buf, t, offset, shape, strides, np_dtype, is_output):
        self.buf, self.t, self.offset, self.shape, self.strides = buf, t, offset, shape, strides
        self.np_dtype, self.is_output = np_dtype, is_output

    @property
    def ptr(self):
        """The address of the view's first element (also when the view is empty)."""
        return self.buf.data_ptr() + self.offset * self.buf.element_size()

    @property
    def ld(self):
        """The larger of the last two strides (the leading dimension of a matrix view)."""
        return max(self.strides[-2:])

    def numpy(self):
        return self.t.cpu().numpy().copy()

    def _inside(self):
        mask = np.zeros(self.buf.numel(), bool)
        if all(self.shape):
            _strided(mask, self.offset, self.shape, self.strides)[...] = True
        return mask

    def touched(self):
        """Buffer offsets outside the view whose bits are no longer the sentinel, relative to the view's
        first element (negative: before it)."""
        assert self.is_output, "only output buffers carry a guard"
        bits = self.buf.view(_SIGNED[self.np_dtype]).cpu().numpy().view(_BITS[self.np_dtype])
        bad = (bits != SENTINEL[self.np_dtype]) & ~self._inside()
        return np.flatnonzero(bad) - self.offset

    def check_guard(self):
        hit = self.touched()
        assert hit.size == 0, ("%d guard element(s) written; the first at offset %+d from the view's first element "
                               "(shape %s, strides %s)" % (hit.size, int(hit[0]), self.shape, self.strides))


def place(array, layout=DENSE, device="cpu", output=False, inout=False):
    """The device operand for `array` (float32 / float64 numpy) under `layout`.  output=True: only the shape
    and dtype of `array` are used.  inout=True: an operand updated in place -- the data inside the view, the
    sentinel (and the guard check) outside it."""
    output = output or inout
    array = np.asarray(array)
    np_dtype = array.dtype
    assert np_dtype in SENTINEL, np_dtype
    offset, strides, length = layout.geometry(array.shape)
    bits = np.full(length, SENTINEL[np_dtype], _BITS[np_dtype])
    host = bits.view(np_dtype)
    if not output:
        host[:] = np.nan
    if (inout or not output) and array.size:
        _strided(host, offset, array.shape, strides)[...] = array
    buf = torch.from_numpy(host).to(device)
    assert buf.data_ptr() % 16 == 0, "the allocator's base is not 16-byte aligned: base_off would mean nothing"
    t = torch.as_strided(buf, array.shape, strides, offset)
    return View(buf, t, offset, tuple(array.shape), tuple(strides), np_dtype, output)


def out_like(shape, np_dtype=np.float32, layout=DENSE, device="cpu"):
    return place(np.empty(shape, np_dtype), layout, device, output=True)


def call_args(view):
    """(pointer, stride, stride, ...) as ``ctx.call`` takes a strided operand: the device address of the first
    element, then the strides in elements in the order of the logical axes."""
    return (view.ptr,) + tuple(view.strides)


def misalignment(view):
    """Elements past a 16-byte boundary of the view's first element."""
    return (view.ptr % 16) // view.buf.element_size()
