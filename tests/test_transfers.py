"""Region transfers without a GPU: ``DeviceArray.copy_region`` / ``set_region`` / ``get_region``
on the fake backend against NumPy indexing (the definition, tests/inputs_transfers.py), what
the case table covers, the error cases, and the argument checks of ``ksp_memcpy_rect_async``,
which come before any device call."""

import ctypes
import types

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from tests import inputs_transfers as it
from tests.fakes import FakeBuffer, FakeContext, FakeQueue

GENERATED_SEED = it.CPU_SEED
GENERATED = it.generate(GENERATED_SEED, 300)


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def merged_shape(case):
    """The byte-level shape that ``_region_transfer_params`` reduces `case` to."""
    context = FakeContext()
    src = accel.DeviceArray(context, case.src_shape, case.dtype, case.src_padded)
    dest = accel.DeviceArray(context, case.dest_shape, case.dtype, case.dest_padded)
    return accel.DeviceArray._region_transfer_params(
        src, dest, case.src_region, case.dest_region)[2]  # fmt: skip


def run_all(context, queue, case, what):
    it.check_copy_region(context, queue, case, what=what + " copy_region")
    it.check_set_region(context, queue, case, plain=False, what=what + " set_region(HostArray)")
    it.check_set_region(context, queue, case, plain=True, what=what + " set_region(ndarray)")
    it.check_get_region(context, queue, case, what=what + " get_region")


# ------------------------------------------------------------------------------- data
class TestData:
    @pytest.mark.parametrize("name", list(it.CASES))
    def test_copy_region(self, name, context, queue):
        it.check_copy_region(context, queue, it.CASES[name])

    @pytest.mark.parametrize("name", list(it.CASES))
    def test_set_region_from_host_array(self, name, context, queue):
        it.check_set_region(context, queue, it.CASES[name], plain=False)

    @pytest.mark.parametrize("name", list(it.CASES))
    def test_set_region_from_ndarray(self, name, context, queue):
        it.check_set_region(context, queue, it.CASES[name], plain=True)

    @pytest.mark.parametrize("name", list(it.CASES))
    def test_get_region(self, name, context, queue):
        it.check_get_region(context, queue, it.CASES[name])

    @pytest.mark.parametrize("block", range(6))
    def test_generated(self, block, context, queue):
        for number in range(block * 50, block * 50 + 50):
            run_all(context, queue, GENERATED[number], f"generated case {number}")

    def test_the_device_tests_cases_stay_inside_their_buffers(self, context, queue):
        """The fake queue refuses a rect copy that leaves a buffer: the cases that
        tests/test_gpu_transfers.py generates are run here first."""
        assert it.GPU_SEED != it.CPU_SEED
        for number, case in enumerate(it.generate(it.GPU_SEED, 100)):
            run_all(context, queue, case, f"device case {number}")

    def test_a_wrong_count_is_noticed(self, context, queue, monkeypatch):
        """The floor count that ``_canonical_slice`` once used fails these tests: on a ragged
        step it drops the last element (equal floor counts on both sides) or finds the two
        sides unequal (a plain ndarray is staged at NumPy's count)."""
        real = accel.DeviceArray._canonical_slice

        def floored(region, shape, strides):
            origin, out_shape, out_strides = real(region, shape, strides)
            items = region if isinstance(region, tuple) else (region,)
            out_shape = list(out_shape)
            position, axis = 0, 0
            for item in items:
                if isinstance(item, slice):
                    start, stop, step = item.indices(shape[axis])
                    out_shape[position] = (stop - start) // step
                if item is np.newaxis or isinstance(item, slice):
                    position += 1
                if item is not np.newaxis:
                    axis += 1
            return origin, tuple(out_shape), out_strides

        monkeypatch.setattr(accel.DeviceArray, "_canonical_slice", staticmethod(floored))
        case = it.CASES["step_ragged_both"]
        with pytest.raises(AssertionError, match="bytes differ"):
            it.check_copy_region(context, queue, case)
        with pytest.raises(AssertionError, match="bytes differ"):
            it.check_set_region(context, queue, case, plain=False)
        with pytest.raises(ValueError, match="shapes for the copy do not match"):
            it.check_set_region(context, queue, case, plain=True)
        it.check_copy_region(context, queue, it.CASES["step_divides"])


# --------------------------------------------------------------------------- the table
# name -> (dimensions after merging, item size, indexing forms): what each row exercises, read
# off _region_transfer_params and the regions. A row that is removed or changed fails this.
PINNED = {
    "0d": (1, 4, ()),
    "1d": (1, 2, ()),
    "2d_rows_merge": (1, 4, ('missing_axes',)),
    "2d_pitched": (2, 8, ()),
    "3d_loop": (3, 1, ()),
    "4d_recurse": (4, 2, ('step',)),
    "5d_recurse": (5, 1, ('step',)),
    "step_divides": (2, 4, ('step',)),
    "step_ragged_inner": (3, 8, ('ragged_inner', 'step')),
    "step_ragged_outer": (2, 1, ('ragged_outer', 'step')),
    "step_ragged_both": (3, 16, ('ragged_inner', 'ragged_outer', 'step')),
    "step_single_element": (1, 2, ('missing_axes', 'ragged_outer', 'single_element_step', 'step')),
    "int_indices": (2, 4, ('int',)),
    "negative_ints": (1, 1, ('negative_bound', 'negative_int')),
    "negative_bounds": (3, 8, ('negative_bound', 'step')),
    "newaxis_src": (1, 16, ('newaxis',)),
    "newaxis_dest": (2, 2, ('newaxis', 'step')),
    "missing_axes": (3, 4, ('missing_axes',)),
    "middle_size_one": (2, 8, ('middle_size_one',)),
    "ref_4d": (4, 4, ('step',)),
    "ref_1d": (1, 4, ('int',)),
    "ref_2d": (1, 4, ('negative_bound',)),
    "ref_missing_axes": (1, 4, ('missing_axes', 'negative_bound')),
    "ref_newaxis": (1, 4, ('newaxis',)),
    "ref_negative": (2, 4, ('negative_bound', 'negative_int', 'step')),
}  # fmt: skip


class TestTable:
    def test_rows_are_the_pinned_ones(self):
        got = {
            name: (len(merged_shape(case)), np.dtype(case.dtype).itemsize,
                   tuple(sorted(it.features(case))))
            for name, case in it.CASES.items()
        }  # fmt: skip
        assert got == PINNED

    def test_coverage(self):
        shapes = {name: merged_shape(case) for name, case in it.CASES.items()}
        assert {len(s) for s in shapes.values()} >= {1, 2, 3, 4, 5}
        assert {np.dtype(c.dtype).itemsize for c in it.CASES.values()} == {1, 2, 4, 8, 16}
        forms = {name: it.features(case) for name, case in it.CASES.items()}
        every = set().union(*forms.values())
        assert every >= {
            "step", "ragged_inner", "ragged_outer", "single_element_step", "newaxis", "int",
            "negative_int", "negative_bound", "missing_axes", "middle_size_one"}  # fmt: skip
        # a step that divides, with no ragged one beside it; ragged on both axes of one case
        assert any("step" in f and not f & {"ragged_inner", "ragged_outer"} for f in forms.values())
        assert any({"ragged_inner", "ragged_outer"} <= f for f in forms.values())
        assert any(f & {"ragged_inner", "ragged_outer"} == {"ragged_inner"} for f in forms.values())
        assert any(f & {"ragged_inner", "ragged_outer"} == {"ragged_outer"} for f in forms.values())
        # newaxis on either side
        assert any(np.newaxis in it._items(c.src_region) for c in it.CASES.values())
        assert any(np.newaxis in it._items(c.dest_region) for c in it.CASES.values())
        # the paths of the rect copy: one run, pitched rows, the loop over planes, the recursion
        assert shapes["0d"] == (4,) and len(shapes["2d_rows_merge"]) == 1
        assert len(shapes["2d_pitched"]) == 2 and len(shapes["3d_loop"]) == 3
        assert len(shapes["4d_recurse"]) == 4 and len(shapes["5d_recurse"]) == 5
        # a stepped innermost axis is copied element by element: rows one element wide
        assert any(s[0] == np.dtype(it.CASES[name].dtype).itemsize and len(s) >= 2
                   for name, s in shapes.items())  # fmt: skip

    def test_sizes_are_small(self):
        for name, case in it.CASES.items():
            for shape, padded in ((case.src_shape, case.src_padded),
                                  (case.dest_shape, case.dest_padded)):  # fmt: skip
                full = it.padded_of(shape, padded)
                assert all(n <= 25 for n in full), name
                n_bytes = int(np.prod(full, dtype=np.int64)) * np.dtype(case.dtype).itemsize
                assert n_bytes <= 128 * 1024, name

    def test_single_element_slice_is_one_element(self):
        origin, shape, strides = accel.DeviceArray._canonical_slice(np.s_[8:10:3], (10,), (4,))
        assert (origin, shape, strides) == (32, (1,), (12,))

    @pytest.mark.parametrize("region, length, count", [
        (np.s_[0:10:3], 10, 4), (np.s_[::2], 5, 3), (np.s_[::4], 9, 3), (np.s_[8:10:3], 10, 1),
        (np.s_[1:7:2], 10, 3),
    ])  # fmt: skip
    def test_counts_are_numpys(self, region, length, count):
        assert len(np.arange(length)[region]) == count
        assert accel.DeviceArray._canonical_slice(region, (length,), (1,))[1] == (count,)


class TestGenerator:
    def test_is_deterministic(self):
        assert it.generate(GENERATED_SEED, 300) == GENERATED
        assert it.generate(GENERATED_SEED, 20) == GENERATED[:20]
        assert it.generate(GENERATED_SEED + 1, 20) != GENERATED[:20]

    def test_cases_are_valid(self):
        for number, case in enumerate(GENERATED):
            assert 1 <= len(case.src_shape) <= 5 and 1 <= len(case.dest_shape) <= 5, number
            assert case.dtype in it.DTYPES
            for shape, padded, region in ((case.src_shape, case.src_padded, case.src_region),
                                          (case.dest_shape, case.dest_padded, case.dest_region)):  # fmt: skip
                full = it.padded_of(shape, padded)
                assert len(full) == len(shape), number
                assert all(1 <= n <= p <= 23 for n, p in zip(shape, full)), number
                assert all(n <= 20 for n in shape), number
                assert int(np.prod(full, dtype=np.int64)) * 16 <= 64 * 1024, number
                for item in it._items(region):
                    if isinstance(item, slice):
                        assert item.step is None or 1 <= item.step <= 4, number
            src = np.empty(case.src_shape, case.dtype)[case.src_region]
            dest = np.empty(case.dest_shape, case.dtype)[case.dest_region]
            assert np.shape(src) == np.shape(dest) and np.size(src) >= 1, number

    def test_cases_are_varied(self):
        assert {len(c.src_shape) for c in GENERATED} == {1, 2, 3, 4, 5}
        assert {len(c.dest_shape) for c in GENERATED} == {1, 2, 3, 4, 5}
        assert {c.dtype for c in GENERATED} == set(it.DTYPES)
        every = set().union(*(it.features(c) for c in GENERATED))
        assert every >= {"step", "ragged_inner", "ragged_outer", "single_element_step", "newaxis",
                         "int", "negative_int", "negative_bound", "missing_axes"}  # fmt: skip
        assert {len(merged_shape(c)) for c in GENERATED} >= {1, 2, 3, 4, 5}
        assert sum(it.is_ragged(c) for c in GENERATED) >= 50
        assert sum(not it.is_ragged(c) for c in GENERATED) >= 50
        assert any(c.src_padded is None for c in GENERATED)


# ------------------------------------------------------------------------------ errors
class TestErrors:
    def attempt(self, context, queue, src_shape, dest_shape, src_region, dest_region,
                src_dtype=np.int32, dest_dtype=np.int32):  # fmt: skip
        src = accel.DeviceArray(context, src_shape, src_dtype)
        dest = accel.DeviceArray(context, dest_shape, dest_dtype)
        src.copy_region(queue, dest, src_region, dest_region)

    @pytest.mark.parametrize("src_region, dest_region, error, message", [
        (np.s_[3, 4], np.s_[5, 6], IndexError, "Too many axes in index expression"),
        (np.s_[5], np.s_[10], IndexError, "Index out of range"),
        (np.s_[-11], np.s_[0], IndexError, "Index out of range"),
        (np.s_[10:12], np.s_[8:10], IndexError, "Empty slice selection"),
        (np.s_[2:2], np.s_[3:3], IndexError, "Empty slice selection"),
        (np.s_[5:2], np.s_[5:2], IndexError, "Empty slice selection"),
        (np.s_[3:0:-1], np.s_[4:1:-1], IndexError, "Only positive strides are supported"),
        (np.s_[0:4:0], np.s_[0:4], ValueError, "slice step cannot be zero"),
        (np.s_[0:3], np.s_[0:4], ValueError, "shapes for the copy do not match"),
        (np.s_[1.5], np.s_[1], TypeError, "Invalid type in slice"),
    ])  # fmt: skip
    def test_bad_regions(self, src_region, dest_region, error, message, context, queue):
        with pytest.raises(error, match=message):
            self.attempt(context, queue, (10,), (10,), src_region, dest_region)
        assert np.empty(10)[2:2].size == 0  # NumPy finds the empty ones empty too

    def test_dtype_mismatch(self, context, queue):
        with pytest.raises(TypeError, match="dtypes do not match"):
            self.attempt(context, queue, (10,), (10,), np.s_[0:3], np.s_[0:3],
                         dest_dtype=np.float32)  # fmt: skip

    def test_nothing_is_copied_on_error(self, context, queue):
        src = accel.DeviceArray(context, (10,), np.int32)
        dest = accel.DeviceArray(context, (10,), np.int32)
        dest.buffer.array[...] = 7
        with pytest.raises(ValueError):
            src.copy_region(queue, dest, np.s_[0:3], np.s_[0:4])
        assert (dest.buffer.array == 7).all()

    def test_host_side_must_be_a_host_array(self, context, queue):
        src = accel.DeviceArray(context, (10,), np.int32)
        with pytest.raises(ValueError, match="not suitable for device-to-host copy"):
            src.get_region(queue, np.zeros(10, np.int32), np.s_[0:3], np.s_[0:3])
        view = accel.HostArray((10,), np.int32)[2:]
        with pytest.raises(ValueError, match="not suitable for device-to-host copy"):
            src.get_region(queue, view, np.s_[0:3], np.s_[0:3])


class TestRectDimensions:
    """1 to 3 dimensions, ValueError otherwise: the fake queue and ``hip.CommandQueue._rect``
    (which raises before it calls the library)."""

    @pytest.mark.parametrize("ndim", [0, 4])
    def test_fake_queue(self, ndim):
        queue = FakeQueue(FakeContext())
        a, b = FakeBuffer((64,), np.uint8), FakeBuffer((64,), np.uint8)
        host = np.zeros(64, np.uint8)
        shape, strides = (1,) * ndim, (1,) * ndim
        with pytest.raises(ValueError, match="1 to 3 dimensions"):
            queue.enqueue_copy_buffer_rect(a, b, 0, 0, shape, strides, strides)
        with pytest.raises(ValueError, match="1 to 3 dimensions"):
            queue.enqueue_read_buffer_rect(a, host, 0, 0, shape, strides, strides)
        with pytest.raises(ValueError, match="1 to 3 dimensions"):
            queue.enqueue_write_buffer_rect(a, host, 0, 0, shape, strides, strides)

    def test_fake_queue_stays_inside_its_buffers(self):
        queue = FakeQueue(FakeContext())
        a, b = FakeBuffer((64,), np.uint8), FakeBuffer((64,), np.uint8)
        queue.enqueue_copy_buffer_rect(a, b, 0, 60, (4,), (1,), (1,))
        with pytest.raises(IndexError):
            queue.enqueue_copy_buffer_rect(a, b, 0, 61, (4,), (1,), (1,))
        with pytest.raises(IndexError):
            queue.enqueue_copy_buffer_rect(a, b, 0, 0, (4, 5), (1, 16), (1, 16))

    def test_fake_queue_copies_what_the_strides_say(self):
        queue = FakeQueue(FakeContext())
        a, b = FakeBuffer((4, 8), np.uint8), FakeBuffer((3, 2, 6), np.uint8)
        a.array[...] = np.arange(32).reshape(4, 8)
        queue.enqueue_copy_buffer_rect(a, b, 9, 1, (2, 2, 3), (1, 4, 8), (1, 6, 12))
        want = np.zeros((3, 2, 6), np.uint8)
        for k in range(3):
            for j in range(2):
                for i in range(2):
                    want[k, j, 1 + i] = 9 + i + 4 * j + 8 * k
        np.testing.assert_array_equal(b.array, want)

    @pytest.mark.parametrize("ndim", [0, 4])
    def test_hip_queue(self, ndim):
        from katsdpsigproc_amd import hip

        context = types.SimpleNamespace(device=types.SimpleNamespace(index=0))
        queue = hip.CommandQueue(context, stream=0)  # a borrowed stream: no device call
        a = types.SimpleNamespace(ptr=256)
        with pytest.raises(ValueError, match="rect copies support 1 to 3 dimensions"):
            queue.enqueue_copy_buffer_rect(a, a, 0, 0, (1,) * ndim, (1,) * ndim, (1,) * ndim)


# ------------------------------------------------------- ksp_memcpy_rect_async's checks
@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_rect_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(256)  # never dereferenced: every call below fails its checks first
    invalid_value = 1  # hipErrorInvalidValue

    def call(ndim=2, kind=2, dst_strides=(1, 16, 64), src_strides=(1, 16, 64)):
        size3 = ctypes.c_size_t * 3
        rc = lib.ksp_memcpy_rect_async(0, p, 0, size3(*dst_strides), p, 0, size3(*src_strides),
                                       size3(4, 2, 1), ndim, kind, None)  # fmt: skip
        assert rc == invalid_value
        return _lib.last_error()

    ndim = "invalid argument: ndim must be 1..3 (ndim >= 1 && ndim <= 3)"
    assert call(ndim=0) == ndim
    assert call(ndim=4) == ndim
    assert call(ndim=-1) == ndim
    kind = "invalid argument: bad copy kind (kind >= 0 && kind <= 2)"
    assert call(kind=3) == kind
    assert call(kind=-1) == kind
    stride = ("invalid argument: innermost stride must be 1 byte "
              "(dst_strides[0] == 1 && src_strides[0] == 1)")  # fmt: skip
    assert call(dst_strides=(2, 16, 64)) == stride
    assert call(src_strides=(4, 16, 64)) == stride
    assert call(dst_strides=(0, 16, 64), src_strides=(0, 16, 64)) == stride
    # the order of the checks
    assert call(ndim=0, kind=3, dst_strides=(2, 16, 64)) == ndim
    assert call(kind=3, dst_strides=(2, 16, 64)) == kind
