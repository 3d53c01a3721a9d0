"""Sub-views for the tests of the C-ABI: a 2-D array with a row stride of its own, some
elements into a larger allocation, with a margin of known bytes before and behind it.

A launcher of ``include/katsdpsigproc_hip.h`` takes raw pointers and row strides, so its caller
may hand it a column block of a wider array or a pointer into the middle of an allocation.
The helpers here build such arrays and afterwards prove that nothing but the rows was written:

* an *output* lies in an allocation full of ``SENTINEL`` bytes, and the reader asserts that
  every byte outside ``[row * stride, row * stride + cols)`` of every row still holds it;
* an *input* lies in an allocation full of poison (NaN for floating-point and complex types,
  0xFF for everything else), so a result that depends on anything outside the rows is wrong.

Each margin is at least one row stride plus 256 bytes long (and a multiple of 256 bytes, so an
`offset` of 0 keeps the first row as aligned as the allocation): an access that strays by up
to a row at either end lands in the margin, inside the allocation, and shows as a wrong
result or a damaged sentinel rather than as an access outside the allocation.

The layout functions work on NumPy arrays alone (tests/test_subviews.py tests them without a
GPU); :class:`DeviceView` and :func:`flat_device_array` / :func:`read_flat` put them on a device.
"""

import contextlib
import ctypes

import numpy as np

SENTINEL = 0xAB
MARGIN_ALIGN = 256


def sentinel_array(padded_shape, dtype):
    """An array of `dtype` whose every byte is ``SENTINEL``."""
    return np.full(padded_shape, SENTINEL, np.uint8).repeat(np.dtype(dtype).itemsize, -1).view(dtype)


def poison_array(n, dtype):
    """`n` elements of what no result may depend on: NaN, or bytes of 0xFF."""
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return np.full(n, complex(np.nan, np.nan), dtype)
    if dtype.kind == "f":
        return np.full(n, np.nan, dtype)
    return np.full(n * dtype.itemsize, 0xFF, np.uint8).view(dtype)


class Layout:
    """Where `shape` = (rows, cols) of `dtype` lies in a flat allocation: rows of `stride`
    elements, the first `offset` elements behind the front margin."""

    def __init__(self, shape, dtype, stride, offset=0):
        self.rows, self.cols = (int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.stride, self.offset = int(stride), int(offset)
        assert self.stride >= self.cols >= 0 and self.rows >= 0 and self.offset >= 0
        itemsize = self.dtype.itemsize
        margin = self.stride * itemsize + 256
        margin = -(-margin // MARGIN_ALIGN) * MARGIN_ALIGN
        self.margin = margin // itemsize  # (in elements: 256 is a multiple of every itemsize)
        self.start = self.margin + self.offset
        # the view ends with the last row's data; the strides behind it belong to the margin
        self.size = self.start + self.rows * self.stride + self.margin

    def view(self, flat):
        """The (rows, cols) data of a flat array of this layout, as a view."""
        assert flat.shape == (self.size,) and flat.dtype == self.dtype
        body = flat[self.start : self.start + self.rows * self.stride]
        return body.reshape(self.rows, self.stride)[:, : self.cols]

    def inside(self):
        """Boolean array over the elements of the allocation: True for the data rows."""
        mask = np.zeros(self.size, bool)
        self.view_of_mask(mask)[...] = True
        return mask

    def view_of_mask(self, mask):
        body = mask[self.start : self.start + self.rows * self.stride]
        return body.reshape(self.rows, self.stride)[:, : self.cols]

    def locate(self, byte):
        """(row, column) of byte number `byte` of the allocation, relative to the view: the
        row is negative in front of the first row, the column counts elements from the start
        of that row (so columns of cols .. stride - 1 are its padding)."""
        element = byte // self.dtype.itemsize - self.start
        return element // self.stride, element % self.stride


def build_host(dtype, data, stride, offset=0, poison=False):
    """(flat host array, layout): `data` (2-D) at its place, every other byte ``SENTINEL``,
    or poison if `poison` (for the inputs of a call)."""
    data = np.asarray(data, dtype)
    assert data.ndim == 2
    layout = Layout(data.shape, dtype, stride, offset)
    flat = poison_array(layout.size, dtype) if poison else sentinel_array((layout.size,), dtype)
    layout.view(flat)[...] = data
    return flat, layout


def check_host(flat, layout, name="array"):
    """The data rows of `flat` (a copy), after asserting that every byte outside them still
    holds the sentinel; the message names the first offending byte as (row, column) of the view."""
    assert flat.shape == (layout.size,) and flat.dtype == layout.dtype
    outside = np.repeat(~layout.inside(), layout.dtype.itemsize)
    bad = np.flatnonzero((flat.view(np.uint8) != SENTINEL) & outside)
    if bad.size:
        row, col = layout.locate(int(bad[0]))
        raise AssertionError(
            f"{name}: {bad.size} bytes outside the rows were written, the first at row {row}, "
            f"column {col} of a view of {layout.rows} x {layout.cols} with stride {layout.stride} "
            f"(byte {int(bad[0])} of the allocation holds {int(flat.view(np.uint8)[bad[0]]):#04x})")  # fmt: skip
    return np.ascontiguousarray(layout.view(flat))


class DeviceView:
    """A sub-view in device memory. ``ptr`` points at element [0][0]; :meth:`read` returns the
    rows after checking everything around them."""

    def __init__(self, context, queue, dtype, data, stride, offset=0, poison=False):
        from katsdpsigproc_amd import accel

        self.queue = queue
        self.host, self.layout = build_host(dtype, data, stride, offset, poison)
        self.poison = poison
        self.array = accel.DeviceArray(context, self.host.shape, dtype)
        assert self.array.buffer.ptr % MARGIN_ALIGN == 0
        queue.enqueue_write_buffer(self.array.buffer, self.host)
        self.address = self.array.buffer.ptr + self.layout.start * self.layout.dtype.itemsize
        self.ptr = ctypes.c_void_p(self.address)
        self.stride = self.layout.stride

    def read(self, name="array"):
        """The rows; every other byte must hold the sentinel (an output) or be what was
        uploaded (an input: nothing may write to it at all)."""
        flat = np.empty(self.host.shape, self.host.dtype)
        self.queue.enqueue_read_buffer(self.array.buffer, flat)
        if self.poison:
            same = flat.view(np.uint8) == self.host.view(np.uint8)
            assert same.all(), f"{name}: an input was written to, first at (row, column) " \
                f"{self.layout.locate(int(np.flatnonzero(~same)[0]))}"  # fmt: skip
            return np.ascontiguousarray(self.layout.view(flat))
        return check_host(flat, self.layout, name)


class CompactViews:
    """The view factory of the raw-ABI tests: ``views(role, dtype, data, stride, offset,
    poison)`` gives (view, pointer to the first element of data), `role` being the name of the
    launcher's argument. Here every view is a :class:`DeviceView` with the stride asked for;
    tests/farviews.py has a factory that moves chosen roles far apart, so the bodies take the
    strides they hand to a launcher from ``view.stride``."""

    def __init__(self, context, queue):
        self.context, self.queue = context, queue

    def __call__(self, role, dtype, data, stride, offset=0, poison=False):
        return flat_device_array(self.context, self.queue, dtype, data, stride, offset, poison)

    def shared_stride(self, like, arrays):
        """The one stride of `arrays`, (role, rows, cols, dtype) each, that a launcher takes
        for several arrays at once: `like`, the compact stride, here."""
        return like

    def mark(self):
        """A point in time for :meth:`release`."""
        return None

    def release(self, mark):
        """The views made since `mark` are done with (a factory with an arena reuses it)."""

    @contextlib.contextmanager
    def scope(self):
        """Views made inside the block are done with at its end."""
        mark = self.mark()
        yield
        self.release(mark)


def flat_device_array(context, queue, dtype, data, stride, offset, poison=False):
    """`data` as a sub-view on the device; returns (view, pointer to the first element of data)."""
    view = DeviceView(context, queue, dtype, data, stride, offset, poison)
    return view, view.ptr


def read_flat(queue, view, shape, stride, offset, name="array"):
    """The data rows of a flat_device_array, after checking every other byte of it. The view
    knows its own layout: `queue`, `shape`, `stride` and `offset` are kept only for the call
    sites of the older tests (test_gpu_average.py), and are checked against it."""
    layout = view.layout
    assert (layout.rows, layout.cols) == tuple(shape)
    assert (layout.stride, layout.offset) == (stride, offset)
    return view.read(name)
