"""Host side of the generic operations, without a GPU: the launch sizes and the size limit of
Fill, and how CommandQueue._enqueue_rtc turns its arguments into what hipModuleLaunchKernel
is given (through a stand-in for the C library's entry point)."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel, fill, hip


# ------------------------------------------------------------------------------- Fill
class RecordingQueue:
    """Records the geometry and arguments of every launch."""

    def __init__(self):
        self.context = object()
        self.launches = []

    def enqueue_kernel(self, kernel, args, global_size=None, local_size=None):
        self.launches.append((kernel, list(args), tuple(global_size), tuple(local_size)))


class StandInProgram:
    def get_kernel(self, name):
        return name


class StandInFillTemplate:
    """What Fill reads of a FillTemplate; nothing is compiled."""

    def __init__(self, dtype, wgs):
        self.dtype = np.dtype(dtype)
        self.ctype = "unused"
        self.wgs = wgs
        self.program = StandInProgram()


class StandInArray:
    """A bound array that owns no memory: the slot validates dtype, shape and padded shape,
    Fill._run reads ``padded_shape`` and ``buffer``."""

    def __init__(self, shape, dtype, padded_shape=None):
        self.shape = tuple(shape)
        self.padded_shape = self.shape if padded_shape is None else tuple(padded_shape)
        self.dtype = np.dtype(dtype)
        self.buffer = object()


def _fill(shape, wgs, dtype=np.uint8):
    queue = RecordingQueue()
    fn = fill.Fill(StandInFillTemplate(dtype, wgs), queue, shape)
    padded = fn.slots["data"].required_padded_shape()
    array = StandInArray(shape, dtype, padded)
    fn.bind(data=array)
    return fn, queue, array


@pytest.mark.parametrize("wgs", [1, 64, 96, 1024])
def test_fill_refuses_two_to_the_32_before_any_launch(wgs):
    fn, queue, _ = _fill((1 << 32,), wgs)
    with pytest.raises(ValueError, match="32-bit"):
        fn()
    assert queue.launches == []
    # the padded shape counts, not the logical one
    fn, queue, _ = _fill((1 << 16, (1 << 16) - 3), wgs)
    assert fn.buffer("data").padded_shape == (1 << 16, 1 << 16)
    with pytest.raises(ValueError, match="32-bit"):
        fn()
    assert queue.launches == []


@pytest.mark.parametrize("wgs", [1, 64, 96, 1024])
def test_fill_largest_count_launches_the_thread_cap(wgs):
    count = (1 << 32) - 1
    fn, queue, array = _fill((count,), wgs)
    fn.set_value(7)
    fn()
    ((kernel, args, global_size, local_size),) = queue.launches
    assert kernel == "fill"
    assert global_size == (wgs * fill._MAX_GROUPS,) and local_size == (wgs,)
    assert fill._MAX_GROUPS == 4096
    assert args[0] is array.buffer
    # the count reaches the kernel whole, as the unsigned int it declares
    assert type(args[1]) is np.uint32 and int(args[1]) == count
    assert type(args[2]) is np.uint8 and args[2] == 7


@pytest.mark.parametrize("wgs", [1, 64, 96, 1024])
@pytest.mark.parametrize("count", [1, 63, 64, 65, 1023, 1024, 1025, 100000])
def test_fill_small_counts_launch_whole_workgroups(count, wgs):
    fn, queue, _ = _fill((count,), wgs)
    fn()
    ((_, args, global_size, local_size),) = queue.launches
    groups = accel.divup(count, wgs)
    assert global_size == (wgs * min(groups, 4096),) and local_size == (wgs,)
    if groups <= 4096:
        assert count <= global_size[0] < count + wgs
    assert int(args[1]) == count


@pytest.mark.parametrize("wgs", [64, 1024])
def test_fill_thread_cap_edges(wgs):
    cap = wgs * 4096
    for count, threads in [(cap - 1, cap), (cap, cap), (cap + 1, cap), (3 * cap + 17, cap)]:
        fn, queue, _ = _fill((count,), wgs)
        fn()
        assert queue.launches[0][2] == (threads,)


def test_fill_counts_padding():
    fn, queue, array = _fill((1000, 33), 64, np.float32)
    assert array.padded_shape == (1000, 64)  # rows of at least 128 bytes round up to them
    fn()
    assert int(queue.launches[0][1][1]) == 64000


def test_fill_kernel_index_is_64_bit():
    text = accel.render_template("fill.hip.in", {"wgs": 64, "ctype": "float"})
    assert "unsigned long long i = get_global_id(0); i < size; i += stride" in text
    assert "const unsigned long long stride = get_global_size(0)" in text
    assert "unsigned int size" in text  # what the host passes as np.uint32


# ---------------------------------------------------------------------------- HReduce
class StandInReduceTemplate:
    def __init__(self, dtype, wgsx, wgsy):
        self.dtype = np.dtype(dtype)
        self.wgsx, self.wgsy = wgsx, wgsy
        self.program = StandInProgram()


@pytest.mark.parametrize("wgsx, wgsy, rows, groups", [(64, 1, 70000, 70000), (16, 4, 70000, 17500),
                                                      (16, 5, 7, 2), (1, 1, 1, 1), (1024, 1, 3, 3)])  # fmt: skip
def test_hreduce_puts_workgroups_on_dimension_x(wgsx, wgsy, rows, groups):
    """One workgroup per wgsy rows, all on grid dimension x (y holds at most 65535)."""
    from katsdpsigproc_amd import reduce

    queue = RecordingQueue()
    fn = reduce.HReduce(StandInReduceTemplate(np.uint32, wgsx, wgsy), queue, (rows, 9), (3, 8))
    for name in ("src", "dest"):
        slot = fn.slots[name]
        fn.bind(**{name: StandInArray(slot.shape, np.uint32, slot.required_padded_shape())})
    fn()
    ((kernel, args, global_size, local_size),) = queue.launches
    assert kernel == "hreduce"
    assert global_size == (wgsx * groups, wgsy) and local_size == (wgsx, wgsy)
    assert groups * wgsy <= fn.buffer("src").padded_shape[0] == fn.buffer("dest").padded_shape[0]
    first, n_cols, stride = args[2:]
    assert [type(a) for a in args[2:]] == [np.int32] * 3
    assert (first, n_cols, stride) == (3, 5, fn.buffer("src").padded_shape[1])


def test_hreduce_refuses_more_threads_than_a_launch_numbers():
    from katsdpsigproc_amd import reduce

    queue = RecordingQueue()
    rows = (1 << 32) // 1024
    fn = reduce.HReduce(StandInReduceTemplate(np.uint8, 1024, 1), queue, (rows, 1))
    for name in ("src", "dest"):
        fn.bind(**{name: StandInArray(fn.slots[name].shape, np.uint8)})
    with pytest.raises(ValueError, match="too many rows"):
        fn()
    assert queue.launches == []


# ----------------------------------------------------------------- kernel arguments
class StandInDevice:
    index = 0


class StandInContext:
    device = StandInDevice()


@pytest.fixture
def launcher(monkeypatch):
    """A CommandQueue on a borrowed stream and a kernel handle, with ``_lib.call`` replaced
    by a recorder: `calls` gets (grid, block, [bytes of each argument]) per launch, the bytes
    read through the parameter pointers with the sizes given in `sizes`."""
    calls, sizes = [], []

    def call(name, *args):
        assert name == "ksp_launch_function"
        device, stream, function, grid, block, shared, params = args
        assert device == 0 and stream.value == 0x1234 and function.value == 0xF00D and shared == 0
        blobs = [ctypes.string_at(params[i], n) for i, n in enumerate(sizes)]
        calls.append((tuple(grid), tuple(block), blobs))
        return 0

    monkeypatch.setattr(hip._lib, "call", call)
    queue = hip.CommandQueue(StandInContext(), stream=0x1234)
    kernel = hip.RtcKernel.__new__(hip.RtcKernel)
    kernel.handle = 0xF00D
    return queue, kernel, calls, sizes


SCALARS = [
    np.int8(-128), np.uint64(2**64 - 1), np.int16(-32768), np.float32(-0.0),
    np.complex128(complex(-0.0, np.nan)), np.bool_(True), np.int64(-(2**63)),
    np.uint16(65535), np.float64(5e-324), np.uint8(255), np.complex64(complex(1.5, -2.25)),
    np.int32(-(2**31)), np.uint32(2**32 - 1), np.uint64(2**53 + 1), np.int64(2**53 + 1),
    np.float32(np.nan), np.float64(np.nan), np.float32(1e-45), np.float32(0.1),
    np.int8(127), np.int16(32767), np.int32(2**31 - 1), np.int64(2**63 - 1),
    np.bool_(False), np.float32(np.inf), np.float64(-np.inf),
]  # fmt: skip


def test_rtc_scalars_are_passed_with_their_own_bytes(launcher):
    """Every scalar dtype, extremes included: the parameter points at exactly the scalar's
    bytes (so 64-bit integers beyond 2^53 did not pass through a float, a complex number is
    (real, imag), -0.0 and NaN keep their bits)."""
    queue, kernel, calls, sizes = launcher
    assert {s.dtype for s in SCALARS} == set(queue._CTYPES) | {np.dtype("c8"), np.dtype("c16")}
    sizes[:] = [s.dtype.itemsize for s in SCALARS]
    queue.enqueue_kernel(kernel, SCALARS, global_size=(64,), local_size=(64,))
    ((grid, block, blobs),) = calls
    assert grid == (1, 1, 1) and block == (64, 1, 1)
    for scalar, blob in zip(SCALARS, blobs):
        assert blob == scalar.tobytes(), scalar.dtype


def test_rtc_pointers(launcher):
    queue, kernel, calls, sizes = launcher

    class Raw:
        ptr, nbytes = 0x7F0000001000, 64

    buffer = hip.Buffer(Raw(), (16,), np.float32)
    raw = hip.RawBuffer.__new__(hip.RawBuffer)
    raw.ptr = 0x7F0000002000
    sizes[:] = [8, 8, 8]
    queue.enqueue_kernel(kernel, [buffer, None, raw], global_size=(8,), local_size=(4,))
    pointers = [int.from_bytes(blob, "little") for blob in calls[0][2]]
    assert pointers == [0x7F0000001000, 0, 0x7F0000002000]


def test_rtc_launch_geometry(launcher):
    queue, kernel, calls, sizes = launcher
    queue.enqueue_kernel(kernel, [], global_size=(8, 6, 4), local_size=(4, 3, 2))
    queue.enqueue_kernel(kernel, [], global_size=(8, 6), local_size=(4, 3))
    queue.enqueue_kernel(kernel, [], global_size=(70000 * 16,), local_size=(16,))
    queue.enqueue_kernel(kernel, [], global_size=(0, 6), local_size=(4, 3))  # nothing to do
    assert [c[:2] for c in calls] == [((2, 2, 2), (4, 3, 2)), ((2, 2, 1), (4, 3, 1)),
                                      ((70000, 1, 1), (16, 1, 1))]  # fmt: skip


def test_rtc_refusals(launcher):
    """What is refused stays refused, with the exception types callers may catch."""
    queue, kernel, calls, _ = launcher
    one = dict(global_size=(64,), local_size=(64,))
    with pytest.raises(TypeError, match="no definite C type"):  # a Python int
        queue.enqueue_kernel(kernel, [4], **one)
    with pytest.raises(TypeError, match="no definite C type"):
        queue.enqueue_kernel(kernel, [1.0], **one)
    with pytest.raises(TypeError, match="float16"):
        queue.enqueue_kernel(kernel, [np.float16(1)], **one)
    with pytest.raises(TypeError, match="longdouble|float128"):
        queue.enqueue_kernel(kernel, [np.longdouble(1)], **one)
    with pytest.raises(ValueError, match="1 to 3 dimensions"):  # 4-D
        queue.enqueue_kernel(kernel, [], global_size=(2, 2, 2, 2), local_size=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="1 to 3 dimensions"):
        queue.enqueue_kernel(kernel, [], global_size=(), local_size=())
    with pytest.raises(ValueError, match="1 to 3 dimensions"):  # ranks differ
        queue.enqueue_kernel(kernel, [], global_size=(4, 4), local_size=(4,))
    with pytest.raises(ValueError, match="multiple"):
        queue.enqueue_kernel(kernel, [], global_size=(100,), local_size=(64,))
    with pytest.raises(ValueError, match="multiple"):
        queue.enqueue_kernel(kernel, [], global_size=(64,), local_size=(0,))
    with pytest.raises(ValueError, match="required"):
        queue.enqueue_kernel(kernel, [], global_size=None, local_size=None)
    with pytest.raises(TypeError, match="not a kernel"):
        queue.enqueue_kernel(object(), [], **one)
    assert calls == []
