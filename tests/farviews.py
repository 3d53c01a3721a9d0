"""Far sub-views: a 2-D array whose row stride is so large that rows lie more than 2**31 and
2**32 bytes behind the pointer a launcher receives, in an allocation of gigabytes of which
only kilobytes are ever copied.

A launcher that computes a row's place with 32-bit arithmetic somewhere -- ``int idx = row *
stride + col``, an ``(unsigned)`` byte offset, a 32-bit ``voffset`` -- passes every test on
small arrays. Truncation is a property of addresses, not of data volume, so a few rows placed
far apart show it. For a row ``r`` of a view with ``stride`` elements of ``itemsize`` bytes

* the byte offset is ``o = r * stride * itemsize`` and
* the element offset is ``i = r * stride``,

and a truncating kernel lands on one of four *aliases* instead of ``o``: the low 32 bits of
``o`` read as unsigned or as signed, or the low 32 bits of ``i`` read as unsigned or as signed,
times ``itemsize``. :class:`FarLayout` places the view in an allocation so that

* every alias of every row lies inside the allocation (the front margin is chosen for it),
* no alias window overlaps a true row's window, and
* every true row has a guard band of ``GUARD`` bytes on both sides,

and asserts all three on the CPU (tests/test_farviews.py). A truncated access therefore stays
inside the allocation and shows as a wrong result or a damaged window, never as a fault.

Like :class:`tests.subviews.DeviceView`, an *input* lies in poison (NaN, 0xFF) -- its rows'
guard bands and every alias window -- and an *output* in ``SENTINEL`` bytes. Only these windows
are uploaded and read back, row by row with plain linear copies. The rest of the allocation is
filled with ``SENTINEL`` by one device memset before the call, and afterwards a small run-time
compiled kernel counts the bytes of the whole allocation that differ from it: the count must
equal the number of such bytes inside the windows, which the host knows from what it read
back. That proves that nothing was written anywhere in the gigabytes between the rows.

The stated limit of these tests: row strides of the C-ABI are ``int`` (``long long`` for
ksp_twodflag and ksp_masked_filter), so an *element* offset reaches 2**31 only where an element
is small or where another array decides. With the allocations used here (a span of a little
over 4 GiB) element offsets of 2**31 and more occur for 1-byte arrays (flags, status, weights8),
where bytes and elements coincide, and for float32 arrays that share their stride with a 1-byte
array when that one chooses it (thresholds, masked filter, 2-D flagger). For 4-, 8- and
16-byte arrays on their own they would need 8 to 32 GiB per array, and only their byte offsets
cross 2**31 and 2**32.
"""

import contextlib
import ctypes

import numpy as np

from katsdpsigproc_amd import hip
from tests.subviews import SENTINEL, poison_array

GUARD = 256
ALIGN = 256
MAX_STRIDE = 2**31 - 1  # strides of the C-ABI are int ...
LONG_STRIDE = 2**62  # ... but for ksp_twodflag and ksp_masked_filter: long long
SPAN = 2**32 + 2**24  # what the rows of a many-row view cover at the least, in bytes


class LayoutError(ValueError):
    """The stride does not allow a layout that meets the three conditions."""


def low32(value):
    """(unsigned, signed) reading of the low 32 bits of `value`."""
    unsigned = value & 0xFFFFFFFF
    return unsigned, unsigned - (1 << 32) if unsigned & 0x80000000 else unsigned


def aliases(row, stride, itemsize):
    """Byte offsets, relative to the pointer, at which a kernel that truncates the byte offset
    or the element offset of `row` to 32 bits lands instead; without the true offset."""
    true = row * stride * itemsize
    found = set(low32(true)) | {i * itemsize for i in low32(row * stride)}
    found.discard(true)
    return sorted(found)


def _merge(intervals):
    merged = []
    for lo, hi in sorted(intervals):
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return [tuple(m) for m in merged]


class FarLayout:
    """Where `shape` = (rows, cols) of `dtype` with rows of `stride` elements lies in an
    allocation of ``size`` bytes: element [0][0] at byte ``start``, `offset` elements behind
    the front margin. ``segments`` are the disjoint byte ranges [lo, hi) of the allocation
    that are ever copied: the windows of the true rows and of their aliases."""

    def __init__(self, shape, dtype, stride, offset=0, max_stride=MAX_STRIDE):
        self.rows, self.cols = (int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.stride, self.offset = int(stride), int(offset)
        itemsize = self.itemsize = self.dtype.itemsize
        if not (self.cols <= self.stride <= max_stride and self.rows >= 1 and self.cols >= 1):
            raise LayoutError(f"stride {stride} for rows of {self.cols} elements")
        assert self.offset >= 0 and GUARD % itemsize == 0
        self.row_bytes = self.cols * itemsize
        self.true = [r * self.stride * itemsize for r in range(self.rows)]
        self.alias = sorted({a for r in range(self.rows) for a in aliases(r, self.stride, itemsize)})
        lowest = min(self.alias + [0])
        front = -(-(GUARD - lowest) // ALIGN) * ALIGN
        self.start = front + self.offset * itemsize
        end = max(self.alias + self.true) + self.row_bytes + GUARD
        self.size = -(-(self.start + end) // ALIGN) * ALIGN

        def window(at):
            return self.start + at - GUARD, self.start + at + self.row_bytes + GUARD

        self.true_windows = [window(o) for o in self.true]
        self.alias_windows = _merge(window(a) for a in self.alias)
        self.segments = _merge(self.true_windows + self.alias_windows)
        self.check()

    def check(self):
        """The three conditions; LayoutError if the stride breaks one."""
        for lo, hi in self.true_windows + self.alias_windows:
            if lo < 0 or hi > self.size:
                raise LayoutError(f"window [{lo}, {hi}) leaves the allocation of {self.size} bytes")
        for (_, hi), (lo, _) in zip(self.true_windows, self.true_windows[1:]):
            if lo < hi:
                raise LayoutError(f"stride {self.stride}: the guard bands of two rows overlap")
        edges = np.array(self.true_windows, np.int64).reshape(-1, 2)
        for lo, hi in self.alias_windows:
            # the true windows are sorted and disjoint: the only candidate is the last that
            # starts below the end of the alias window
            k = int(np.searchsorted(edges[:, 0], hi)) - 1
            if k >= 0 and edges[k, 1] > lo:
                raise LayoutError(
                    f"stride {self.stride}: the alias window [{lo}, {hi}) overlaps row {k}")

    def row_slices(self):
        """For every row, (index into segments, slice of that segment's bytes) of its data."""
        los = np.array([lo for lo, _ in self.segments], np.int64)
        found = []
        for o in self.true:
            at = self.start + o
            k = int(np.searchsorted(los, at, side="right")) - 1
            found.append((k, slice(at - self.segments[k][0], at - self.segments[k][0] + self.row_bytes)))
        return found

    def image(self, data, poison):
        """The bytes of every segment before the call: `data` in its rows, poison around them
        and in the alias windows if `poison` (an input), else ``SENTINEL`` (an output)."""
        data = np.ascontiguousarray(data, self.dtype)
        assert data.shape == (self.rows, self.cols)
        chunks = []
        for lo, hi in self.segments:
            assert (lo - self.start) % self.itemsize == 0 and (hi - lo) % self.itemsize == 0
            if poison:
                chunks.append(poison_array((hi - lo) // self.itemsize, self.dtype).view(np.uint8).copy())
            else:
                chunks.append(np.full(hi - lo, SENTINEL, np.uint8))
        for row, (k, where) in zip(data, self.row_slices()):
            chunks[k][where] = row.view(np.uint8)
        return chunks

    def rows_of(self, chunks):
        """The (rows, cols) data in the segment bytes `chunks`, as a new array."""
        out = np.empty((self.rows, self.row_bytes), np.uint8)
        for r, (k, where) in enumerate(self.row_slices()):
            out[r] = chunks[k][where]
        return out.view(self.dtype)

    def outside(self):
        """Per segment, a boolean array: True for the bytes that belong to no row."""
        masks = [np.ones(hi - lo, bool) for lo, hi in self.segments]
        for k, where in self.row_slices():
            masks[k][where] = False
        return masks

    def locate(self, byte):
        """(row, column) of byte `byte` of the allocation relative to the view, as
        :meth:`tests.subviews.Layout.locate` gives them."""
        element = (byte - self.start) // self.itemsize
        return element // self.stride, element % self.stride


def check_segments(layout, before, after, poison, name="array"):
    """The rows read back, after asserting that an input's windows are untouched, or that an
    output's guard bands and alias windows still hold the sentinel."""
    for (lo, _), was, now, outside in zip(layout.segments, before, after, layout.outside()):
        bad = np.flatnonzero(now != was) if poison else np.flatnonzero((now != SENTINEL) & outside)
        if bad.size:
            row, col = layout.locate(lo + int(bad[0]))
            kind = "an input was written to" if poison else "bytes outside the rows were written"
            raise AssertionError(
                f"{name}: {kind}, {bad.size} in one window, the first at row {row}, column {col} "
                f"of a view of {layout.rows} x {layout.cols} with stride {layout.stride} "
                f"(byte {lo + int(bad[0])} of the allocation holds {int(now[bad[0]]):#04x})")
    return layout.rows_of(after)


def expected_count(chunks):
    """What the audit must count in the whole allocation: the bytes of the segments (which are
    disjoint) that differ from the sentinel. Everything else was memset and never touched."""
    return sum(int(np.count_nonzero(chunk != SENTINEL)) for chunk in chunks)


def far_stride(rows, cols, dtype, like, span=SPAN, max_stride=MAX_STRIDE):
    """A far stride, in elements, for `rows` rows of `cols` elements whose compact test uses
    the stride `like`: the same residue modulo 16 elements (so rows on 16-byte boundaries stay
    there, odd strides stay odd, even ones that are no multiple of 16 stay so), and

    * a byte stride of 2**32 plus that small remainder where up to three rows of 4-byte or
      wider elements allow it: every byte alias is a small positive offset, no front margin;
    * else the smallest stride with which the rows span more than 2**32 bytes; rows between
      2**31 and 2**32 have negative signed aliases, so the front margin is 2**31 bytes;
    * with so few rows of so small elements that not even the largest ``int`` stride spans
      that, the largest one: the view goes as far as its shape lets it.

    `span` is what the rows are to cover (a view that cannot afford 2**32 bytes asks for a
    little over 2**31), `max_stride` the largest stride the launcher's argument holds. Where
    the first two both apply, the one with the smaller allocation is taken. Strides the
    layout has to reject (an alias that falls on another row) are stepped over."""
    itemsize = np.dtype(dtype).itemsize
    residue = like % 16
    if rows < 2:
        return like  # a single row has nowhere to go
    candidates = []
    if rows <= 3 and itemsize >= 4 and span > 2**32:
        candidates.append((2**32 // itemsize + up16(cols) + residue, 16))
    spanning = up16(max(like, -(-span // ((rows - 1) * itemsize)))) + residue
    if spanning <= max_stride:
        candidates.append((spanning, 16))
    else:
        candidates.append(((max_stride // 16 - 1) * 16 + residue, -16))
    best = None
    for stride, step in candidates:
        for _ in range(64):
            try:
                layout = FarLayout((rows, cols), dtype, stride, 0, max_stride)
            except LayoutError:
                stride += step
                continue
            if best is None or layout.size < best.size:
                best = layout
            break
    if best is None:
        raise LayoutError(f"no far stride for {rows} x {cols} of {np.dtype(dtype)}")
    return best.stride


def up16(n):
    return -(-n // 16) * 16


COUNT_SOURCE = """
extern "C" __global__ void count_not_sentinel(const uint4 *data, unsigned long long n_vectors,
                                              unsigned long long *count)
{
    const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long found = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
         i < n_vectors; i += step) {
        const uint4 v = data[i];
        const unsigned int words[4] = {v.x, v.y, v.z, v.w};
        for (int w = 0; w < 4; w++)
            for (int b = 0; b < 4; b++)
                found += ((words[w] >> (8 * b)) & 0xffu) != ${sentinel}u;
    }
    if (found != 0) atomicAdd(count, found);
}
"""


class Arena:
    """One large device allocation that the far views of a test share, slice after slice;
    :meth:`reset` hands all of it out again. Skips the test if the device cannot give it."""

    def __init__(self, context, queue, n_bytes):
        import pytest

        from katsdpsigproc_amd import accel

        self.context, self.queue = context, queue
        self.device = context.device.index
        try:
            self.raw = context.allocate_raw(n_bytes)
        except RuntimeError as exc:
            if "memory" not in str(exc).lower():
                raise
            pytest.skip(f"the device could not allocate {n_bytes} bytes for far views: {exc}")
        assert self.raw.ptr % ALIGN == 0
        self.n_bytes, self.used, self.peak = n_bytes, 0, 0
        program = accel.build(context, "count_not_sentinel", {"sentinel": str(SENTINEL)},
                              source=COUNT_SOURCE)  # fmt: skip
        self.kernel = program.get_kernel("count_not_sentinel")
        self.counter = accel.DeviceArray(context, (1,), np.uint64)

    def reset(self):
        self.used = 0

    def take(self, n_bytes):
        """Address of `n_bytes` (a multiple of 256) of the arena, full of sentinel bytes."""
        assert n_bytes % ALIGN == 0
        assert self.used + n_bytes <= self.n_bytes, \
            f"far views of {self.used + n_bytes} bytes in an arena of {self.n_bytes}"  # fmt: skip
        address = self.raw.ptr + self.used
        self.used += n_bytes
        self.peak = max(self.peak, self.used)
        self.call("ksp_memset_async", ctypes.c_void_p(address), SENTINEL, n_bytes, self.stream)
        return address

    @property
    def stream(self):
        return ctypes.c_void_p(self.queue.stream)

    def call(self, name, *args):
        from katsdpsigproc_amd import _lib

        return _lib.call(name, self.device, *args)

    def copy(self, address, chunks, to_device):
        """Linear copies between host `chunks` and the device addresses `address`."""
        for at, chunk in zip(address, chunks):
            host, dev = ctypes.c_void_p(chunk.ctypes.data), ctypes.c_void_p(at)
            if to_device:
                self.call("ksp_memcpy_async", dev, host, chunk.nbytes, 0, self.stream)
            else:
                self.call("ksp_memcpy_async", host, dev, chunk.nbytes, 1, self.stream)
        self.queue.finish()

    def count(self, address, n_bytes):
        """Bytes of [address, address + n_bytes) that differ from the sentinel."""
        assert address % 16 == 0 and n_bytes % 16 == 0
        self.counter.zero(self.queue)
        data = BorrowedBuffer(self.device, address, n_bytes)
        self.queue.enqueue_kernel(self.kernel, [data, np.uint64(n_bytes // 16), self.counter.buffer],
                                  global_size=(256 * 2048,), local_size=(256,))  # fmt: skip
        return int(self.counter.get(self.queue)[0])


class BorrowedBuffer(hip.RawBuffer):
    """Device memory that belongs to someone else (a slice of an :class:`Arena`) with the
    public surface of ``hip.RawBuffer`` -- ``ptr``, ``nbytes``, ``device_index`` -- so that it
    serves as a kernel argument or as the ``raw`` of a ``DeviceArray``. It allocates nothing and
    frees nothing: the owner must outlive it."""

    def __init__(self, device_index, ptr, n_bytes):  # (no call of the allocating constructor)
        self.device_index, self.ptr, self.nbytes = device_index, int(ptr), int(n_bytes)


class FarDeviceView:
    """A far sub-view in an :class:`Arena`, with the surface of
    :class:`tests.subviews.DeviceView`: ``ptr`` points at element [0][0], :meth:`read` returns
    the rows after checking their windows and auditing the whole allocation."""

    def __init__(self, arena, dtype, data, stride, offset=0, poison=False, max_stride=MAX_STRIDE):
        self.arena, self.poison = arena, poison
        data = np.asarray(data, dtype)
        self.layout = FarLayout(data.shape, dtype, stride, offset, max_stride)
        self.base = arena.take(self.layout.size)
        self.before = self.layout.image(data, poison)
        self.where = [self.base + lo for lo, _ in self.layout.segments]
        arena.copy(self.where, self.before, to_device=True)
        self.address = self.base + self.layout.start
        self.ptr = ctypes.c_void_p(self.address)
        self.stride = self.layout.stride

    @property
    def reach(self):
        """Byte offset of the last row from ``ptr``."""
        return self.layout.true[-1]

    def read(self, name="array"):
        after = [np.empty_like(chunk) for chunk in self.before]
        self.arena.copy(self.where, after, to_device=False)
        rows = check_segments(self.layout, self.before, after, self.poison, name)
        counted = self.arena.count(self.base, self.layout.size)
        assert counted == expected_count(after), \
            (f"{name}: {counted} bytes of the allocation of {self.layout.size} differ from the "
             f"sentinel, {expected_count(after)} of them inside the windows of the rows: "
             "something was written between the rows")  # fmt: skip
        return rows


FAR_SPAN = 1 << 26  # rows that span as many bytes lie in the arena, whatever their role


class FarViews:
    """The view factory of :class:`tests.subviews.CompactViews` with the arrays of the roles
    `far` far: each gets a far stride of the same alignment class as the stride asked for and
    lies in `arena`; every other array is what `compact` makes of it. `span` and `max_stride`
    are those of :func:`far_stride`."""

    def __init__(self, arena, far, compact, span=SPAN, max_stride=MAX_STRIDE):
        self.arena, self.far, self.compact, self.made = arena, frozenset(far), compact, set()
        self.span, self.max_stride = span, max_stride
        arena.reset()

    @staticmethod
    def spans(rows, stride, dtype):
        return (rows - 1) * stride * np.dtype(dtype).itemsize >= FAR_SPAN

    def __call__(self, role, dtype, data, stride, offset=0, poison=False):
        rows, cols = np.shape(data)
        if role in self.far and not self.spans(rows, stride, dtype):
            stride = far_stride(rows, cols, dtype, stride, self.span, self.max_stride)
        if not self.spans(rows, stride, dtype):
            return self.compact(role, dtype, data, stride, offset, poison)
        self.made.add(role)
        view = FarDeviceView(self.arena, dtype, data, stride, offset, poison, self.max_stride)
        return view, view.ptr

    def shared_stride(self, like, arrays):
        """A far stride that suits every array that shares it, chosen for the far ones: the
        narrowest far type decides, so that its rows cover the span too."""
        chosen = [far_stride(rows, cols, dtype, like, self.span, self.max_stride)
                  for role, rows, cols, dtype in arrays if role in self.far]  # fmt: skip
        if not chosen:
            return like
        stride = max(chosen)
        # upwards, or downwards from the largest stride an int holds (where a wider type's
        # alias falls just short of the row before)
        step = 16 if stride + 512 * 16 <= self.max_stride else -16
        for _ in range(512):
            try:
                for _, rows, cols, dtype in arrays:
                    FarLayout((rows, cols), dtype, stride, 0, self.max_stride)
                return stride
            except LayoutError:
                stride += step
        raise LayoutError(f"no shared far stride near {stride}")

    def mark(self):
        return self.arena.used

    def release(self, mark):
        """The views made since `mark` give their part of the arena back."""
        self.arena.used = mark

    @contextlib.contextmanager
    def scope(self):
        mark = self.mark()
        yield
        self.release(mark)

    def check(self):
        """Every role that was asked to be far was (a misspelt role would pass unnoticed)."""
        assert self.made >= self.far, f"far views of {sorted(self.made)}, asked for {sorted(self.far)}"
