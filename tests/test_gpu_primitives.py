"""Fill, HReduce and the launch path under them (CommandQueue._enqueue_rtc) on the GPU, at
every element type and at the sizes where they could go wrong: more elements than threads
(the grid stride of fill), partly filled wavefronts and rows at lane offsets (hreduce), more
rows than one grid dimension numbers, scalars of every type in an order that mixes sizes.
Everything is compared with NumPy on whole padded buffers, bit for bit unless a summation
order differs, and padding and unselected columns hold values that would show if read."""

import functools
import os

import numpy as np
import pytest

from katsdpsigproc_amd import accel

pytestmark = pytest.mark.gpu

KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels")
GUARD = 4096  # bytes behind an array that must stay untouched
FILLER = 0xA5  # byte in memory that a kernel is expected to overwrite, or to leave alone


@pytest.fixture(scope="module")
def context():
    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def pad_dimension(dim, extra):
    """Force at least `extra` elements of padding (as in test_gpu_ops.py)."""
    accel.Dimension(dim.size, min_padded_size=dim.size + extra).link(dim)


def _bits(ary):
    """The bytes of `ary`, so that NaN equals NaN and -0.0 differs from 0.0."""
    return np.ascontiguousarray(ary).reshape(-1).view(np.uint8)


def _write_bytes(command_queue, buffer, value=FILLER):
    command_queue.enqueue_write_buffer(buffer, np.full(buffer.nbytes, value, np.uint8))


def _read(command_queue, buffer, shape=None, dtype=None):
    out = np.empty(buffer.shape if shape is None else shape, buffer.dtype if dtype is None else dtype)
    command_queue.enqueue_read_buffer(buffer, out)
    return out


# ------------------------------------------------------------------------------- Fill
F32, F64 = np.float32, np.float64
FILL_TYPES = {
    "unsigned char": (np.uint8, [0, 255, 0x3C]),
    "short": (np.int16, [-32768, 32767, -2]),
    "unsigned int": (np.uint32, [0, 2**32 - 1, 0xDEADBEEF]),
    "long long": (np.int64, [-(2**63), 2**63 - 1, 2**53 + 1]),
    "float": (F32, [F32(-0.0), F32(np.inf), F32(np.nan), F32(1e-45), F32(0.1)]),
    "double": (F64, [F64(-0.0), F64(np.inf), F64(np.nan), F64(5e-324), F64(0.1)]),
    "float2": (np.complex64, [np.complex64(complex(1.5, -2.25)), np.complex64(complex(-0.0, np.nan)),
                              np.complex64(complex(np.inf, 1e-45))]),
    "double2": (np.complex128, [np.complex128(complex(1.5, -2.25)),
                                np.complex128(complex(-0.0, np.nan)),
                                np.complex128(complex(np.inf, 5e-324))]),
}  # fmt: skip


@functools.lru_cache(maxsize=None)
def _fill_template(context, ctype, wgs):
    from katsdpsigproc_amd import fill

    return fill.FillTemplate(context, FILL_TYPES[ctype][0], ctype, tuning={"wgs": wgs})


def test_fill_value_patterns():
    """What the value lists are meant to hold (a check of this file, not of the kernel)."""
    assert F32(1e-45).view(np.uint32) == 1 and F64(5e-324).view(np.uint64) == 1
    assert F32(-0.0).view(np.uint32) == 0x80000000 and F32(np.nan).view(np.uint32) == 0x7FC00000
    assert F64(np.nan).view(np.uint64) == 0x7FF8000000000000
    assert F32(0.1).view(np.uint32) == 0x3DCCCCCD


@pytest.mark.parametrize("shape, pad", [((75,), 0), ((75, 63), 0), ((3, 5, 7), 0), ((1000, 33), 5)],
                         ids=["75", "75x63", "3x5x7", "1000x33+5"])  # fmt: skip
@pytest.mark.parametrize("ctype", list(FILL_TYPES))
def test_fill_types_and_values(ctype, shape, pad, context, command_queue):
    """Every element size, on padded arrays of 1 to 3 dimensions: the whole padded buffer
    holds exactly the value's bits, for each value in turn through one operation (the value
    is an argument of the launch, not part of the compiled kernel)."""
    dtype, values = FILL_TYPES[ctype]
    fn = _fill_template(context, ctype, 64).instantiate(command_queue, shape)
    if pad:
        pad_dimension(fn.slots["data"].dimensions[-1], pad)
    fn.ensure_all_bound()
    data = fn.buffer("data")
    assert data.padded_shape[-1] >= shape[-1] + pad
    _write_bytes(command_queue, data.buffer)
    assert len(values) >= 3
    for value in values:
        fn.set_value(value)
        assert fn.value.dtype == dtype
        fn()
        got = _read(command_queue, data.buffer, data.padded_shape)
        expected = np.full(data.padded_shape, value, dtype)
        np.testing.assert_array_equal(_bits(got), _bits(expected), err_msg=repr(value))


CAP64 = 64 * 4096  # threads of one launch at wgs=64
FILL_SIZES = [(64, n) for n in (1, 63, 64, 65, CAP64 - 1, CAP64, CAP64 + 1, 3 * CAP64 + 17)]


@pytest.mark.parametrize(
    "ctype, wgs, count",
    [(ctype, wgs, n) for ctype in ("unsigned char", "float2") for wgs, n in FILL_SIZES]
    + [("unsigned char", 1024, 1024 * 4096 + 1)],
)
def test_fill_sizes_and_guard(ctype, wgs, count, context, command_queue):
    """Around the workgroup size and around the thread cap of wgs * 4096, beyond which
    threads take more than one element each: every element is written and the 4096 bytes
    behind the array are not. The array sits at the start of a larger raw allocation."""
    dtype, values = FILL_TYPES[ctype]
    fn = _fill_template(context, ctype, wgs).instantiate(command_queue, (count,))
    slot = fn.slots["data"]
    n_bytes = slot.required_bytes()
    assert n_bytes == count * np.dtype(dtype).itemsize
    raw = context.allocate_raw(n_bytes + GUARD)
    whole = context.allocate((n_bytes + GUARD,), np.uint8, raw=raw)
    _write_bytes(command_queue, whole)
    data = slot.allocate(fn.allocator, raw=raw)
    assert data.buffer.ptr == whole.ptr and fn.buffer("data") is data
    value = values[2]
    assert FILLER not in _bits(np.asarray(value, dtype))  # an element left out shows
    fn.set_value(value)
    fn()
    got = _read(command_queue, whole)
    np.testing.assert_array_equal(got[:n_bytes], _bits(np.full(count, value, dtype)))
    assert (got[n_bytes:] == FILLER).all(), "wrote behind the array"


def test_fill_unsupported_scalar_is_refused(context, command_queue):
    """A dtype whose scalars cannot be passed to a kernel is accepted by the template (which
    only pastes the C type's name, here one of the same size) and refused at launch."""
    from katsdpsigproc_amd import fill

    template = fill.FillTemplate(context, np.float16, "unsigned short", tuning={"wgs": 64})
    fn = template.instantiate(command_queue, (8,))
    fn.set_value(1.0)
    with pytest.raises(TypeError, match="float16"):
        fn()


# ---------------------------------------------------------------------------- HReduce
GEOMETRIES = [(1, 1), (1, 64), (2, 32), (16, 5), (32, 3), (64, 1), (64, 16), (128, 8), (512, 2),
              (1024, 1)]  # fmt: skip


class Reduction:
    """One operator on one element type: how to compile it, data for it, the value that
    would change a result if a kernel read it, and NumPy's answer."""

    def __init__(self, dtype, ctype, op, identity, poison, draw, expected, extra_code=""):
        self.dtype, self.ctype, self.op, self.identity = np.dtype(dtype), ctype, op, identity
        self.poison, self.draw, self.expected, self.extra_code = poison, draw, expected, extra_code


def _float_helper(name, call):
    return f"DEVICE_FN static inline float {name}(float a, float b) {{ return {call}(a, b); }}"


REDUCTIONS = {
    # sums that wrap: values near 2^31
    "uint32-sum": Reduction(
        np.uint32, "unsigned int", "a + b", "0", 0xFFFFFFFF,
        lambda rs, shape: rs.randint(2**31 - 1000, 2**31 + 1000, shape).astype(np.uint32),
        lambda x: x.sum(axis=1, dtype=np.uint32)),
    "int64-sum": Reduction(
        np.int64, "long long", "a + b", "0", 0xFFFFFFFF,
        lambda rs, shape: rs.randint(-(2**40), 2**40 + 1, shape, dtype=np.int64),
        lambda x: x.sum(axis=1, dtype=np.int64)),
    # bit 7 is never set in the data: the poison would set it
    "uint8-or": Reduction(
        np.uint8, "unsigned char", "a | b", "0", 0xFF,
        lambda rs, shape: (1 << rs.randint(0, 7, shape)).astype(np.uint8),
        lambda x: np.bitwise_or.reduce(x, axis=1)),
    "int16-min": Reduction(
        np.int16, "short", "min(a, b)", "32767", -32768,
        lambda rs, shape: rs.randint(-32767, 32768, shape).astype(np.int16),
        lambda x: x.min(axis=1)),
    # integer-valued floats: every partial sum is exact, so the order cannot matter
    "float-sum": Reduction(
        np.float32, "float", "a + b", "0.0f", np.inf,
        lambda rs, shape: rs.randint(-999, 1000, shape).astype(np.float32),
        lambda x: x.sum(axis=1, dtype=np.float64).astype(np.float32)),
    "double-sum": Reduction(
        np.float64, "double", "a + b", "0.0", np.inf,
        lambda rs, shape: rs.randint(-999, 1000, shape).astype(np.float64),
        lambda x: x.sum(axis=1)),
    "float-fmin": Reduction(
        np.float32, "float", "lo(a, b)", "INFINITY", -np.inf,
        lambda rs, shape: rs.standard_normal(shape).astype(np.float32),
        lambda x: x.min(axis=1), _float_helper("lo", "fminf")),
    "float-fmax": Reduction(
        np.float32, "float", "hi(a, b)", "-INFINITY", np.inf,
        lambda rs, shape: rs.standard_normal(shape).astype(np.float32),
        lambda x: x.max(axis=1), _float_helper("hi", "fmaxf")),
}  # fmt: skip


@functools.lru_cache(maxsize=None)
def _reduce_template(context, name, wgsx, wgsy):
    from katsdpsigproc_amd import reduce

    r = REDUCTIONS[name]
    return reduce.HReduceTemplate(context, r.dtype, r.ctype, r.op, r.identity, r.extra_code,
                                  tuning={"wgsx": wgsx, "wgsy": wgsy})  # fmt: skip


def _layouts(wgsx, wgsy):
    """(rows, columns, (first, last)) for one geometry: row counts around wgsy, range lengths
    around wgsx, ranges that start at column 0 and at 3, and end before and at the last
    column."""
    row_counts = sorted({1, wgsy - 1, wgsy + 1, 7} - {0})
    lengths = sorted({1, wgsx - 1, wgsx, wgsx + 1, 2 * wgsx + 3} - {0})
    for rows in row_counts:
        for n_cols in lengths:
            for first in (0, 3):
                for tail in (0, 2):
                    yield rows, first + n_cols + tail, (first, first + n_cols)


def _run_reduce(context, command_queue, template, poison, data, column_range, calls=1):
    """HReduce of `data` over `column_range`. The src rows are padded by 5 more than the
    slot asks; padding, padding rows and the columns outside the range hold `poison`; dest
    is overwritten beforehand, so that a row the kernel misses cannot hold an old answer.
    Returns the result of each call."""
    rows, columns = data.shape
    first, last = column_range
    fn = template.instantiate(command_queue, (rows, columns), column_range)
    pad_dimension(fn.slots["src"].dimensions[1], 5)
    fn.ensure_all_bound()
    src, dest = fn.buffer("src"), fn.buffer("dest")
    assert src.padded_shape[0] % template.wgsy == 0 and src.padded_shape[1] >= columns + 5
    host = np.full(src.padded_shape, poison, data.dtype)
    host[:rows, first:last] = data[:, first:last]
    command_queue.enqueue_write_buffer(src.buffer, host)
    results = []
    for _ in range(calls):
        _write_bytes(command_queue, dest.buffer)
        fn()
        results.append(np.array(dest.get(command_queue)))
    return results


@pytest.mark.parametrize("wgsx, wgsy", GEOMETRIES)
@pytest.mark.parametrize("name", list(REDUCTIONS))
def test_hreduce_exact(name, wgsx, wgsy, context, command_queue):
    """Every operator and type at every geometry and layout, equal to NumPy on the selected
    columns (all of these are exact in any order)."""
    r = REDUCTIONS[name]
    template = _reduce_template(context, name, wgsx, wgsy)
    rs = np.random.RandomState(wgsx * 64 + wgsy)
    for rows, columns, column_range in _layouts(wgsx, wgsy):
        data = r.draw(rs, (rows, columns))
        assert data.dtype == r.dtype
        (got,) = _run_reduce(context, command_queue, template, r.poison, data, column_range)
        first, last = column_range
        expected = r.expected(data[:, first:last])
        assert got.dtype == expected.dtype and got.shape == (rows,)
        np.testing.assert_array_equal(got, expected,
                                      err_msg=f"{rows} x {columns}, columns {column_range}")  # fmt: skip


@pytest.mark.parametrize("wgsx, wgsy", GEOMETRIES)
@pytest.mark.parametrize("name, wide, u", [("float-sum", np.float64, 2.0**-24),
                                           ("double-sum", np.longdouble, 2.0**-53)])  # fmt: skip
def test_hreduce_float_sum(name, wide, u, wgsx, wgsy, context, command_queue):
    """Sums of standard-normal data: the kernel adds in another order than NumPy, so the
    result is compared with the sum in a wider type. Any order of n - 1 additions with one
    rounding each is within (n - 1) u sum|x| of the true sum to first order; the bound used
    is n u sum|x| per row (u = 2^-24 or 2^-53), which also covers the higher-order terms
    and the wider sum's own rounding. Two calls give the same bits."""
    r = REDUCTIONS[name]
    assert np.finfo(wide).eps < u * 2**-8
    template = _reduce_template(context, name, wgsx, wgsy)
    rs = np.random.RandomState(wgsx * 64 + wgsy + 1)
    for rows, columns, column_range in _layouts(wgsx, wgsy):
        data = rs.standard_normal((rows, columns)).astype(r.dtype)
        once, twice = _run_reduce(context, command_queue, template, r.poison, data, column_range,
                                  calls=2)  # fmt: skip
        first, last = column_range
        selected = data[:, first:last].astype(wide)
        expected = selected.sum(axis=1)
        bound = (last - first) * u * np.abs(selected).sum(axis=1)
        error = np.abs(once.astype(wide) - expected)
        where = f"{rows} x {columns}, columns {column_range}"
        assert np.isfinite(once).all(), where
        assert (error <= bound).all(), f"{where}: {error} > {bound}"
        np.testing.assert_array_equal(_bits(once), _bits(twice), err_msg=where)


@pytest.mark.parametrize("wgsx, wgsy", [(64, 1), (16, 4)])
def test_hreduce_many_rows(wgsx, wgsy, context, command_queue):
    """More workgroups of rows than grid dimensions y and z number (65535): 70000 rows at one
    row per workgroup, and 17500 workgroups of four rows as the control. With the workgroups
    on dimension y the first launch was refused ("invalid argument"); they are on x now."""
    name = "uint32-sum"
    template = _reduce_template(context, name, wgsx, wgsy)
    data = REDUCTIONS[name].draw(np.random.RandomState(3), (70000, 5))
    (got,) = _run_reduce(context, command_queue, template, 0xFFFFFFFF, data, (0, 5))
    np.testing.assert_array_equal(got, data.sum(axis=1, dtype=np.uint32))


# ------------------------------------------------------------------- kernel arguments
# in the order of the kernel's parameters (tests/kernels/args_test.hip.in)
ARG_TYPES = [np.int8, np.uint64, np.int16, np.float32, np.complex128, np.bool_, np.int64,
             np.uint16, np.float64, np.uint8, np.complex64, np.int32, np.uint32]  # fmt: skip
ARG_VALUES = [
    # minima, all-ones, -0.0; complex numbers whose halves differ
    [-128, 2**64 - 1, -32768, -0.0, complex(-0.0, np.nan), True, -(2**63), 65535, -0.0, 255,
     complex(1.5, -2.25), -(2**31), 2**32 - 1],
    # maxima, NaN; 64-bit integers that no float64 holds
    [127, 2**53 + 1, 32767, np.nan, complex(1.5, -2.25), False, 2**63 - 1, 0, np.nan, 0,
     complex(np.nan, -0.0), 2**31 - 1, 0],
    [-1, 2**63 + 1, 1, np.finfo(np.float32).max, complex(np.inf, 5e-324), True, -(2**53) - 1,
     0x1234, np.finfo(np.float64).max, 0x12, complex(-np.inf, 1e-45), 0x12345678, 0x9ABCDEF0],
]  # fmt: skip


@pytest.fixture(scope="module")
def args_program(context):
    return accel.build(context, "args_test.hip.in", {}, extra_dirs=[KERNELS])


def test_arg_types_cover_the_queue(command_queue):
    assert {np.dtype(t) for t in ARG_TYPES} == (
        set(command_queue._CTYPES) | {np.dtype(np.complex64), np.dtype(np.complex128)})  # fmt: skip


@pytest.mark.parametrize("values", ARG_VALUES, ids=["min", "max", "other"])
@pytest.mark.parametrize("with_pointer", [False, True], ids=["null", "pointer"])
def test_scalar_arguments(values, with_pointer, context, command_queue, args_program):
    """One scalar of every type enqueue_kernel passes by value, sizes interleaved: each
    arrives with exactly its bits. A None argument arrives as a null pointer."""
    scalars = [np.array(v).astype(t)[()] for v, t in zip(values, ARG_TYPES)]
    assert [s.dtype for s in scalars] == [np.dtype(t) for t in ARG_TYPES]
    outputs = [accel.DeviceArray(context, (1,), np.uint8 if t is np.bool_ else t) for t in ARG_TYPES]
    is_null = accel.DeviceArray(context, (1,), np.int32)
    for out in outputs + [is_null]:
        _write_bytes(command_queue, out.buffer)
    pointer = accel.DeviceArray(context, (1,), np.int32).buffer if with_pointer else None
    command_queue.enqueue_kernel(
        args_program.get_kernel("scalars"),
        scalars + [pointer] + [out.buffer for out in outputs] + [is_null.buffer],
        global_size=(64,), local_size=(64,))  # fmt: skip
    for scalar, out in zip(scalars, outputs):
        got = _read(command_queue, out.buffer)
        assert _bits(got).tobytes() == scalar.tobytes(), f"{scalar.dtype}: {got[0]!r} != {scalar!r}"
    assert _read(command_queue, is_null.buffer)[0] == (2 if with_pointer else 1)


def test_launch_3d(context, command_queue, args_program):
    out = accel.DeviceArray(context, (4, 6, 8), np.int32)
    _write_bytes(command_queue, out.buffer)
    command_queue.enqueue_kernel(args_program.get_kernel("grid3d"), [out.buffer],
                                 global_size=(8, 6, 4), local_size=(4, 3, 2))  # fmt: skip
    z, y, x = np.indices((4, 6, 8))
    np.testing.assert_array_equal(out.get(command_queue), z * 10000 + y * 100 + x)
