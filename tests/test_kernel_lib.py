"""The helper headers for run-time compiled kernels on the GPU: kernels/wg_reduce.h,
transpose_base.h and rank.h, through the test kernels of tests/kernels/ built by
accel.build. Inputs are chosen so that every comparison is exact: integers, or floats
that hold small integers, wherever the order of a summation could matter."""

import os

import numpy as np
import pytest

from katsdpsigproc_amd import accel

pytestmark = pytest.mark.gpu

KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels")


@pytest.fixture(scope="module")
def context():
    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def _flag(value):
    return "true" if value else "false"


def _device(context, command_queue, ary, padded_shape=None):
    out = accel.DeviceArray(context, ary.shape, ary.dtype, padded_shape)
    if padded_shape is not None:
        out.zero(command_queue)
    out.set(command_queue, ary)
    return out


# ----------------------------------------------------------------------------- reduce
SIZES = [1, 4, 12, 16, 32, 64, 87, 97, 128, 160, 192, 256, 1024]


def _rows(size):
    return max(1, 256 // size)


def _build_reduce(context, ctype, size, op, op2, broadcast, shuffle):
    keys = {"type": ctype, "size": size, "rows": _rows(size), "op": op, "op2": op2,
            "broadcast": _flag(broadcast), "shuffle": _flag(shuffle)}  # fmt: skip
    return accel.build(context, "reduce_test.hip.in", keys, extra_dirs=[KERNELS])


def _run_reduce(context, command_queue, program, name, data, n_out=1):
    """Launch kernel `name` as one work-group of size x rows work-items on `data`
    (rows, size); returns n_out arrays of that shape."""
    rows, size = data.shape[:2]
    src = _device(context, command_queue, data)
    outs = [accel.DeviceArray(context, data.shape, data.dtype) for _ in range(n_out)]
    for out in outs:
        out.zero(command_queue)
    command_queue.enqueue_kernel(program.get_kernel(name), [src.buffer] + [o.buffer for o in outs],
                                 global_size=(size, rows), local_size=(size, rows))  # fmt: skip
    return [np.asarray(o.get(command_queue)) for o in outs]


def _check_reduce(got, expected, broadcast):
    """`expected` has one entry per partition: every work-item holds it, or idx 0 alone."""
    if broadcast:
        np.testing.assert_array_equal(got, np.broadcast_to(expected[:, None], got.shape))
    else:
        np.testing.assert_array_equal(got[:, 0], expected)


@pytest.mark.parametrize("broadcast", [True, False])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("size", SIZES)
def test_reduce_int(size, shuffle, broadcast, context, command_queue):
    program = _build_reduce(context, "int", size, "op_plus", "op_max", broadcast, shuffle)
    data = np.random.RandomState(size).randint(-100000, 100000, (_rows(size), size)).astype(np.int32)
    (total,) = _run_reduce(context, command_queue, program, "reduce", data)
    _check_reduce(total, data.sum(axis=1, dtype=np.int32), broadcast)
    (largest,) = _run_reduce(context, command_queue, program, "reduce2", data)
    _check_reduce(largest, data.max(axis=1), broadcast)
    # both through one scratch, back to back
    total, largest = _run_reduce(context, command_queue, program, "reduce_twice", data, 2)
    _check_reduce(total, data.sum(axis=1, dtype=np.int32), broadcast)
    _check_reduce(largest, data.max(axis=1), broadcast)


@pytest.mark.parametrize("broadcast", [True, False])
@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("size", [12, 64, 160, 256])
@pytest.mark.parametrize("ctype, dtype", [("long long", np.int64), ("double", np.float64),
                                          ("float2", np.complex64)])  # fmt: skip
def test_reduce_wide_types(ctype, dtype, size, shuffle, broadcast, context, command_queue):
    program = _build_reduce(context, ctype, size, "op_plus", "op_plus", broadcast, shuffle)
    rs = np.random.RandomState(size)
    shape = (_rows(size), size)
    if dtype == np.int64:
        # sums that need all 64 bits
        data = rs.randint(-(2**40), 2**40, shape).astype(np.int64)
    elif dtype == np.complex64:
        data = (rs.randint(-1000, 1000, shape) + 1j * rs.randint(-1000, 1000, shape)).astype(dtype)
    else:
        data = rs.randint(-(2**30), 2**30, shape).astype(dtype)
    total, again = _run_reduce(context, command_queue, program, "reduce_twice", data, 2)
    _check_reduce(total, data.sum(axis=1, dtype=dtype), broadcast)
    _check_reduce(again, data.sum(axis=1, dtype=dtype), broadcast)


@pytest.mark.parametrize("shuffle", [True, False])
@pytest.mark.parametrize("size", [12, 64, 87, 160])
def test_reduce_fmin_fmax_ignore_nan(size, shuffle, context, command_queue):
    program = _build_reduce(context, "float", size, "op_fmin", "op_fmax", True, shuffle)
    rs = np.random.RandomState(size)
    rows = _rows(size)
    data = rs.standard_normal((rows, size)).astype(np.float32)
    data[rs.random_sample(data.shape) < 0.4] = np.nan
    data[0, 0] = np.nan  # idx 0 itself starts from NaN
    data[0, 1] = 0.5
    lo, hi = _run_reduce(context, command_queue, program, "reduce_twice", data, 2)
    _check_reduce(lo, np.nanmin(data, axis=1), True)
    _check_reduce(hi, np.nanmax(data, axis=1), True)
    # nothing but NaN gives NaN
    data[:] = np.nan
    lo, hi = _run_reduce(context, command_queue, program, "reduce_twice", data, 2)
    assert np.isnan(lo).all() and np.isnan(hi).all()


# ------------------------------------------------------------------------------- rank
RANK_SIZE = 128
STORE = 8


@pytest.fixture(scope="module", params=[True, False], ids=["shuffle", "lds"])
def rank_program(request, context):
    keys = {"size": RANK_SIZE, "store": STORE, "shuffle": _flag(request.param)}
    return accel.build(context, "rank_test.hip.in", keys, extra_dirs=[KERNELS])


def _shared(context, command_queue, program, name, data, extra=(), n_out=1):
    """One work-group of RANK_SIZE work-items on the 1-D float32 array `data`."""
    data = np.asarray(data, np.float32)
    src = _device(context, command_queue, data)
    out = accel.DeviceArray(context, (n_out,), np.float32)
    out.zero(command_queue)
    command_queue.enqueue_kernel(program.get_kernel(name),
                                 [src.buffer, np.int32(len(data))] + list(extra) + [out.buffer],
                                 global_size=(RANK_SIZE,), local_size=(RANK_SIZE,))  # fmt: skip
    return np.asarray(out.get(command_queue))


@pytest.fixture(scope="module")
def counts():
    data = np.random.RandomState(1).randint(0, 1000, 2000).astype(np.int32)
    expected = (data[None, :] < np.arange(1000)[:, None]).sum(axis=1).astype(np.int32)
    expected.setflags(write=False)
    return data, expected


@pytest.mark.parametrize("name, work_items", [("rank_serial", 1), ("rank_parallel", RANK_SIZE)])
def test_count_below(name, work_items, counts, rank_program, context, command_queue):
    data, expected = counts
    src = _device(context, command_queue, data)
    out = accel.DeviceArray(context, (1000,), np.int32)
    out.zero(command_queue)
    command_queue.enqueue_kernel(rank_program.get_kernel(name),
                                 [src.buffer, np.int32(len(data)), np.int32(1000), out.buffer],
                                 global_size=(work_items,), local_size=(work_items,))  # fmt: skip
    np.testing.assert_array_equal(out.get(command_queue), expected)


@pytest.mark.parametrize("case", ["single", "nan_among", "uniform_sorted", "uniform", "all_nan"])
def test_min_max(case, rank_program, context, command_queue):
    data = {
        "single": [5.3],
        "nan_among": [-10, 5.5, np.nan, -20, np.nan],
        "uniform_sorted": np.sort(np.random.RandomState(2).uniform(-5, 5, 1000)),
        "uniform": np.random.RandomState(2).uniform(-5, 5, 1000),
        "all_nan": [np.nan] * 300,
    }[case]
    data = np.asarray(data, np.float32)
    got = _shared(context, command_queue, rank_program, "minmax", data, n_out=2)
    if case == "all_nan":
        assert np.isnan(got).all()
    else:
        np.testing.assert_array_equal(got, [np.nanmin(data), np.nanmax(data)])


def _median_case(case):
    rs = np.random.RandomState(3)
    if case == "single":
        return [5.3]
    if case == "four":
        return [2.5, 1.25, 7.0, 3.5]
    if case == "zeros_first":
        return [0.0, 0.0, 0.0, 1.2, 1.3, 1.1]
    if case in ("odd_many", "even_many"):
        data = rs.uniform(0.5, 1.5, 10001 if case == "odd_many" else 10000)
        data[4321] = 0.0
        return data
    assert case == "tied_middle"
    return [3.0, 1.0, 2.0, 2.0, 5.0, 2.0]


@pytest.mark.parametrize("case", ["single", "four", "zeros_first", "odd_many", "even_many", "tied_middle"])
def test_median_non_zero(case, rank_program, context, command_queue):
    data = np.asarray(_median_case(case), np.float32)
    expected = np.median(data[data > 0])
    assert expected.dtype == np.float32
    got = _shared(context, command_queue, rank_program, "median", data)
    assert got[0] == expected


@pytest.mark.parametrize("which, halfway", [("first", False), ("last", False), ("middle", False),
                                            ("middle", True)])  # fmt: skip
def test_find_rank(which, halfway, rank_program, context, command_queue):
    data = np.random.RandomState(4).uniform(0.001, 1000.0, 1000).astype(np.float32)
    ordered = np.sort(data)
    rank = {"first": 0, "last": len(data) - 1, "middle": 487}[which]
    expected = (ordered[rank] + ordered[rank - 1]) * np.float32(0.5) if halfway else ordered[rank]
    got = _shared(context, command_queue, rank_program, "find_rank", data,
                  extra=[np.int32(rank), np.int32(halfway)])  # fmt: skip
    assert got[0] == expected


@pytest.mark.parametrize("halfway", [False, True])
def test_find_rank_each_work_item_on_its_own(halfway, rank_program, context, command_queue):
    # not uniform: 192 work-items, 7 values and a middle rank each (one place is NaN padding)
    rs = np.random.RandomState(5)
    items, n = 192, STORE - 1
    data = rs.uniform(0.001, 1000.0, (items, n)).astype(np.float32)
    ranks = rs.randint(1, n, items).astype(np.int32)
    ordered = np.sort(data, axis=1)
    at = ordered[np.arange(items), ranks]
    below = ordered[np.arange(items), ranks - 1]
    expected = (at + below) * np.float32(0.5) if halfway else at
    out = accel.DeviceArray(context, (items,), np.float32)
    command_queue.enqueue_kernel(
        rank_program.get_kernel("find_rank_each"),
        [_device(context, command_queue, data).buffer, np.int32(n),
         _device(context, command_queue, ranks).buffer, np.int32(halfway), out.buffer],
        global_size=(items,), local_size=(64,))  # fmt: skip
    np.testing.assert_array_equal(out.get(command_queue), expected)


def test_median_each_work_item_on_its_own(rank_program, context, command_queue):
    # not uniform: four values each, zeros among them in some rows
    rs = np.random.RandomState(6)
    items, n = 192, 4
    data = rs.uniform(0.5, 1.5, (items, n)).astype(np.float32)
    data[::3, 1] = 0.0
    data[::5, 3] = 0.0
    expected = np.array([np.median(row[row > 0]) for row in data], np.float32)
    out = accel.DeviceArray(context, (items,), np.float32)
    command_queue.enqueue_kernel(rank_program.get_kernel("median_each"),
                                 [_device(context, command_queue, data).buffer, np.int32(n), out.buffer],
                                 global_size=(items,), local_size=(64,))  # fmt: skip
    np.testing.assert_array_equal(out.get(command_queue), expected)


# -------------------------------------------------------------------------- transpose
SHAPES = [(4, 5), (53, 7), (53, 81), (32, 64), (65, 130), (1, 300), (300, 1)]
TILINGS = [(8, 1, 1), (8, 2, 3), (16, 4, 1), (32, 2, 2)]
ELEMENTS = [("unsigned char", np.uint8), ("unsigned short", np.uint16), ("float", np.float32),
            ("float2", np.complex64), ("double2", np.complex128)]  # fmt: skip


def _random(rs, shape, dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "c":
        return (rs.randint(-50, 50, shape) + 1j * rs.randint(-50, 50, shape)).astype(dtype)
    return rs.randint(0, 200, shape).astype(dtype)


def _run_transpose(context, command_queue, kernel, tiling, data, out_dtype):
    """Source stride padded by 4 elements, destination stride by 3; returns the whole
    padded destination, which was zero before the launch."""
    block, vtx, vty = tiling
    rows, cols = data.shape
    src = _device(context, command_queue, data, (rows, cols + 4))
    dest = accel.DeviceArray(context, (cols, rows), out_dtype, (cols, rows + 3))
    dest.zero(command_queue)
    command_queue.enqueue_kernel(
        kernel,
        [src.buffer, dest.buffer, np.int32(rows), np.int32(cols), np.int32(cols + 4), np.int32(rows + 3)],
        global_size=(accel.divup(cols, block * vtx) * block, accel.divup(rows, block * vty) * block),
        local_size=(block, block))  # fmt: skip
    raw = np.empty(dest.padded_shape, out_dtype)
    command_queue.enqueue_read_buffer(dest.buffer, raw)
    return raw


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("ctype, dtype", ELEMENTS, ids=[str(np.dtype(d).itemsize) for _, d in ELEMENTS])
def test_transpose_copy(ctype, dtype, tiling, context, command_queue):
    keys = dict(zip(("block", "vtx", "vty"), tiling), ctype=ctype)
    kernel = accel.build(context, "transpose_test.hip.in", keys, extra_dirs=[KERNELS]).get_kernel("transpose_copy")
    rs = np.random.RandomState(7)
    for rows, cols in SHAPES:
        data = _random(rs, (rows, cols), dtype)
        raw = _run_transpose(context, command_queue, kernel, tiling, data, dtype)
        np.testing.assert_array_equal(raw[:, :rows], data.T, err_msg=str((rows, cols)))
        assert not raw[:, rows:].any(), "wrote into the destination's padding"


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda t: "x".join(map(str, t)))
def test_transpose_fused(tiling, context, command_queue):
    keys = dict(zip(("block", "vtx", "vty"), tiling), ctype="float")
    kernel = accel.build(context, "transpose_test.hip.in", keys, extra_dirs=[KERNELS]).get_kernel("transpose_power")
    rs = np.random.RandomState(8)
    for rows, cols in SHAPES:
        data = _random(rs, (rows, cols), np.complex64)
        raw = _run_transpose(context, command_queue, kernel, tiling, data, np.float32)
        expected = (data.real**2 + data.imag**2).astype(np.float32).T
        np.testing.assert_array_equal(raw[:, :rows], expected, err_msg=str((rows, cols)))
        assert not raw[:, rows:].any(), "wrote into the destination's padding"
