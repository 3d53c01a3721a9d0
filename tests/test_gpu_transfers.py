"""The layer under every kernel test, on the device: ``accel.DeviceArray``'s transfers and
``hip.CommandQueue``'s copies, events and borrowed streams.

Region copies are compared byte for byte with NumPy indexing on host arrays (the definition,
tests/inputs_transfers.py) over the destination's whole padded buffer: every byte outside the
region must keep the sentinel it held before. Nothing here moves more than kilobytes, except
the transposes of the timing checks. Timing bounds come from the definition alone: the time
between two events of a stream cannot exceed the host's wall-clock time around the enqueues
and the ``finish()`` that enclose them.
"""

import gc
import time

import numpy as np
import pytest

from tests import inputs_transfers as it

pytestmark = pytest.mark.gpu

GENERATED = it.generate(it.GPU_SEED, 100)


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def queue(context):
    return context.create_command_queue()


# ---------------------------------------------------------------------- region transfers
class TestRegions:
    @pytest.mark.parametrize("name", list(it.CASES))
    def test_copy_region(self, name, context, queue):
        it.check_copy_region(context, queue, it.CASES[name])
        queue.finish()

    @pytest.mark.parametrize("blocking", [True, False])
    @pytest.mark.parametrize("name", list(it.CASES))
    def test_set_region(self, name, blocking, context, queue):
        case = it.CASES[name]
        it.check_set_region(context, queue, case, plain=False, blocking=blocking, pinned=context)
        it.check_set_region(context, queue, case, plain=True, blocking=blocking)

    @pytest.mark.parametrize("blocking", [True, False])
    @pytest.mark.parametrize("name", list(it.CASES))
    def test_get_region(self, name, blocking, context, queue):
        case = it.CASES[name]
        it.check_get_region(context, queue, case, blocking=blocking, pinned=context)
        it.check_get_region(context, queue, case, blocking=blocking, pinned=None)

    @pytest.mark.parametrize("blocking", [True, False])
    @pytest.mark.parametrize("block", range(4))
    def test_generated(self, block, blocking, context, queue):
        for number in range(block * 25, block * 25 + 25):
            case = GENERATED[number]
            what = f"generated case {number} (blocking={blocking}) "
            it.check_copy_region(context, queue, case, what=what + "copy_region")
            it.check_set_region(context, queue, case, plain=False, blocking=blocking,
                                pinned=context, what=what + "set_region(HostArray)")  # fmt: skip
            it.check_set_region(context, queue, case, plain=True, blocking=blocking,
                                what=what + "set_region(ndarray)")  # fmt: skip
            it.check_get_region(context, queue, case, blocking=blocking, pinned=context,
                                what=what + "get_region(pinned)")  # fmt: skip
            it.check_get_region(context, queue, case, blocking=blocking, pinned=None,
                                what=what + "get_region(pageable)")  # fmt: skip

    def test_asynchronous_regions_hold_their_host_memory(self, context):
        """A non-blocking region copy keeps its host side alive until ``finish()``: the
        pinned staging copy of a plain ndarray has no other owner."""
        queue = context.create_command_queue()
        case = it.CASES["step_ragged_both"]
        src_full, dest_full, expected = it.host_images(case)
        dest = it.upload(context, queue, case.dest_shape, case.dest_padded, dest_full)
        dest.set_region(queue, it.window(src_full, case.src_shape), case.dest_region,
                        case.src_region, blocking=False)  # fmt: skip
        assert queue._keepalive
        queue.finish()
        assert not queue._keepalive
        it.same_bytes(expected, it.download(queue, dest), "set_region(ndarray), not blocking")


# ----------------------------------------------------------------- whole-array transfers
WHOLE_SHAPES = [
    ((), ()),
    ((13,), (16,)),
    ((5, 7), (6, 9)),
    ((3, 4, 5), (4, 4, 7)),
    ((2, 3, 4, 5), (3, 3, 5, 6)),
]


class TestWholeArrays:
    @pytest.mark.parametrize("dtype", it.DTYPES)
    @pytest.mark.parametrize("shape, padded", WHOLE_SHAPES)
    def test_round_trips(self, shape, padded, dtype, context, queue):
        from katsdpsigproc_amd import accel

        data = it.values(shape, dtype, seed=len(shape) + 1)
        image = it.filled(padded, dtype, it.SENTINEL)
        it.window(image, shape)[...] = data
        # a matching HostArray goes up and comes back as it is, padding included
        for asynchronous in (False, True):
            array = accel.DeviceArray(context, shape, dtype, padded)
            assert array.strides == image.strides
            host = it.host_array(shape, padded, image, context)
            if asynchronous:
                array.set_async(queue, host)
                queue.finish()
            else:
                array.set(queue, host)
            it.same_bytes(image, it.download(queue, array), "set(HostArray)")
            if asynchronous:
                back = array.get_async(queue)
                queue.finish()
            else:
                back = array.get(queue)
            assert isinstance(back, accel.HostArray) and back.padded_shape == tuple(padded)
            it.same_bytes(image, accel.HostArray.padded_view(back), "get()")
            it.same_bytes(np.asarray(data), np.asarray(back), "get() window")
        # a plain ndarray is staged: its values arrive (the padding is nobody's)
        for asynchronous in (False, True):
            array = accel.DeviceArray(context, shape, dtype, padded)
            if asynchronous:
                array.set_async(queue, np.array(data))
                queue.finish()
            else:
                array.set(queue, np.array(data))
            it.same_bytes(np.asarray(data), it.window(it.download(queue, array), shape),
                          "set(ndarray)")  # fmt: skip

    def test_get_reuses_a_matching_host_array_only(self, context, queue):
        from katsdpsigproc_amd import accel

        array = accel.DeviceArray(context, (5, 7), np.float32, (6, 9))
        data = it.values((5, 7), np.float32, seed=3)
        array.set(queue, data)
        match = array.empty_like()
        assert array.get(queue, match) is match
        np.testing.assert_array_equal(match, data)
        match[...] = 0
        assert array.get_async(queue, match) is match
        queue.finish()
        np.testing.assert_array_equal(match, data)
        others = [
            np.zeros((5, 7), np.float32),  # no HostArray
            accel.HostArray((5, 7), np.float32, (6, 10), context=context),  # other padding
            accel.HostArray((5, 7), np.int32, (6, 9), context=context),  # other dtype
            accel.HostArray((5, 6), np.float32, (6, 9), context=context),  # other shape
            accel.HostArray((6, 9), np.float32, context=context)[:5, :7],  # a view
        ]
        for other in others:
            for get in (array.get, array.get_async):
                got = get(queue, other)
                queue.finish()
                assert got is not other and isinstance(got, accel.HostArray)
                assert got.padded_shape == (6, 9) and got.dtype == np.float32
                np.testing.assert_array_equal(got, data)

    @pytest.mark.parametrize("dtype", it.DTYPES)
    def test_zero_clears_the_padding_too(self, dtype, context, queue):
        image = it.filled((4, 5, 7), dtype, it.SENTINEL)
        array = it.upload(context, queue, (3, 4, 5), (4, 5, 7), image)
        array.zero(queue)
        assert not it.download(queue, array).view(np.uint8).any()

    def test_whole_buffer_copies_check_the_host_array(self, context):
        queue = context.create_command_queue()
        image = it.filled((6, 8), np.float32, it.SENTINEL)
        array = it.upload(context, queue, (6, 8), None, image)
        wide = np.zeros((6, 16), np.float32)
        for blocking in (True, False):
            for bad, message in [
                (wide[:, :8], "C-contiguous"),
                (np.zeros((6, 8), np.float32).T, "C-contiguous"),
                (np.zeros((6, 7), np.float32), "differ in size"),
                (np.zeros((6, 8), np.float64), "differ in size"),
                (memoryview(bytes(192)), "C-contiguous numpy array"),
            ]:
                with pytest.raises(ValueError, match=message):
                    queue.enqueue_write_buffer(array.buffer, bad, blocking=blocking)
                with pytest.raises(ValueError, match=message):
                    queue.enqueue_read_buffer(array.buffer, bad, blocking=blocking)
                assert not queue._keepalive
        assert not wide.any()  # nothing was read into it
        it.same_bytes(image, it.download(queue, array), "after refused copies")


# ------------------------------------------------------------ lifetime of async copies
class TestLifetime:
    def test_set_async_keeps_a_temporary_alive(self, context):
        from katsdpsigproc_amd import accel

        queue = context.create_command_queue()
        array = accel.DeviceArray(context, (64, 100), np.float32, (64, 128))
        array.set_async(queue, np.arange(6400, dtype=np.float32).reshape(64, 100) * 3)
        gc.collect()
        assert len(queue._keepalive) == 1
        # allocations that would take the staging buffer's place had it been released
        spare = [accel.HostArray((64, 100), np.float32, (64, 128), context=context)
                 for _ in range(4)]  # fmt: skip
        for host in spare:
            accel.HostArray.padded_view(host)[...] = -1
        queue.finish()
        assert queue._keepalive == []
        got = array.get(queue)
        np.testing.assert_array_equal(got, np.arange(6400, dtype=np.float32).reshape(64, 100) * 3)

    def test_get_async_is_kept_until_finish(self, context):
        from katsdpsigproc_amd import accel

        queue = context.create_command_queue()
        array = accel.DeviceArray(context, (9, 5), np.int16, (10, 8))
        data = it.values((9, 5), np.int16, seed=5)
        array.set(queue, data)
        assert queue._keepalive == []
        got = array.get_async(queue)
        assert len(queue._keepalive) == 1
        assert queue._keepalive[0] is accel.HostArray.padded_view(got)
        queue.finish()
        assert queue._keepalive == []
        np.testing.assert_array_equal(got, data)

    def test_release_host_references_does_not_synchronise(self, context, monkeypatch):
        from katsdpsigproc_amd import _lib, accel

        queue = context.create_command_queue()
        array = accel.DeviceArray(context, (9, 5), np.int16, (10, 8))
        host = array.empty_like()  # stays alive in this frame until the finish() below
        host[...] = it.values((9, 5), np.int16, seed=6)
        array.set_async(queue, host)
        back = array.get_async(queue)
        assert len(queue._keepalive) == 2
        calls = []
        real = _lib.call
        monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append(name) or real(name, *args))
        queue.release_host_references()
        assert "ksp_stream_synchronize" not in calls and queue._keepalive == []
        queue.finish()
        assert calls.count("ksp_stream_synchronize") == 1
        np.testing.assert_array_equal(back, host)


# ------------------------------------------------------------------------- raw storage
class TestRawStorage:
    def test_two_arrays_on_one_allocation(self, context, queue):
        from katsdpsigproc_amd import accel

        raw = context.allocate_raw(256)
        floats = accel.DeviceArray(context, (8, 6), np.float32, (8, 8), raw=raw)
        octets = accel.DeviceArray(context, (256,), np.uint8, raw=raw)
        assert floats.buffer.ptr == octets.buffer.ptr == raw.ptr
        image = it.filled((8, 8), np.float32, it.SENTINEL)
        it.window(image, (8, 6))[...] = it.values((8, 6), np.float32, seed=7)
        floats.set(queue, it.host_array((8, 6), (8, 8), image, context))
        np.testing.assert_array_equal(octets.get(queue), image.reshape(-1).view(np.uint8))
        octets.set(queue, np.arange(256, dtype=np.uint8))
        np.testing.assert_array_equal(
            accel.HostArray.padded_view(floats.get(queue)),
            np.arange(256, dtype=np.uint8).view(np.float32).reshape(8, 8))  # fmt: skip

    def test_alias_slot(self, context, queue):
        from katsdpsigproc_amd import accel

        wide = accel.IOSlot((4, 5), np.complex64)
        narrow = accel.IOSlot((30,), np.int16)
        alias = accel.AliasIOSlot([wide, narrow])
        assert alias.required_bytes() == 160
        raw = alias.allocate(accel.DeviceAllocator(context))
        assert raw.nbytes >= 160
        assert wide.buffer.buffer.ptr == narrow.buffer.buffer.ptr == raw.ptr
        data = it.values((4, 5), np.complex64, seed=8)
        wide.buffer.set(queue, data)
        np.testing.assert_array_equal(narrow.buffer.get(queue), data.reshape(-1).view(np.int16)[:30])
        shorts = it.values((30,), np.int16, seed=9)
        narrow.buffer.set(queue, shorts)
        got = wide.buffer.get(queue)
        np.testing.assert_array_equal(np.asarray(got).reshape(-1).view(np.int16)[:30], shorts)
        np.testing.assert_array_equal(np.asarray(got).reshape(-1).view(np.int16)[30:],
                                      data.reshape(-1).view(np.int16)[30:])  # fmt: skip

    def test_raw_storage_must_be_large_enough(self, context):
        from katsdpsigproc_amd import accel

        raw = context.allocate_raw(255)
        accel.DeviceArray(context, (63,), np.float32, raw=raw)
        with pytest.raises(ValueError, match="raw storage is smaller than the requested array"):
            accel.DeviceArray(context, (64,), np.float32, raw=raw)
        with pytest.raises(ValueError, match="raw storage is smaller than the requested array"):
            accel.DeviceArray(context, (8, 6), np.float32, (8, 8), raw=raw)

    def test_shared_virtual_memory_is_not_provided(self, context):
        with pytest.raises(NotImplementedError):
            context.allocate_svm((4,), np.float32)
        with pytest.raises(NotImplementedError):
            context.allocate_svm_raw(16)


# ------------------------------------------------------------- events and tuning queue
def transposes(context, queue, rows=1024, cols=1024):
    """(operation, its input on the host): a float32 transpose bound and run once."""
    from katsdpsigproc_amd import transpose

    fn = transpose.TransposeTemplate(context, np.float32, "float").instantiate(queue, (rows, cols))
    fn.ensure_all_bound()
    data = np.random.RandomState(11).standard_normal((rows, cols)).astype(np.float32)
    fn.buffer("src").set(queue, data)
    fn()
    queue.finish()
    return fn, data


class TestEvents:
    def test_markers_time_the_work_between_them(self, context):
        queue = context.create_command_queue()
        fn, data = transposes(context, queue)
        begin = time.perf_counter()
        first = queue.enqueue_marker()
        for _ in range(20):
            fn()
        last = queue.enqueue_marker()
        queue.finish()
        wall = time.perf_counter() - begin
        elapsed = last.time_since(first)
        print(f"20 transposes of 1024 x 1024 float32: {elapsed * 1e6:.1f} us between the events, "
              f"{wall * 1e6:.1f} us on the host")  # fmt: skip
        assert isinstance(elapsed, float)
        assert 0 < elapsed <= wall
        assert first.time_till(last) == last.time_since(first) == elapsed
        np.testing.assert_array_equal(fn.buffer("dest").get(queue), data.T)

    def test_wait_returns_after_the_work(self, context):
        queue = context.create_command_queue()
        fn, data = transposes(context, queue)
        fn.buffer("dest").zero(queue)
        for _ in range(20):
            fn()
        host = fn.buffer("dest").get_async(queue)
        event = queue.enqueue_marker()
        event.wait()  # (no finish(): the event alone says that the copy is complete)
        np.testing.assert_array_equal(host, data.T)
        queue.release_host_references()
        assert queue._keepalive == []

    def test_wait_for_events_orders_two_queues(self, context):
        first = context.create_command_queue()
        second = context.create_command_queue()
        fn, data = transposes(context, first)
        fn.buffer("dest").zero(first)
        for _ in range(20):
            fn()
        second.enqueue_wait_for_events([first.enqueue_marker()])
        np.testing.assert_array_equal(fn.buffer("dest").get(second), data.T)
        first.finish()

    def test_create_event(self, context, queue):
        from katsdpsigproc_amd import hip

        event = queue.create_event()
        assert isinstance(event, hip.Event) and event.handle
        assert event.handle != queue.create_event().handle

    def test_tuning_queue(self, context):
        from katsdpsigproc_amd import hip

        queue = context.create_tuning_command_queue()
        assert isinstance(queue, hip.TuningCommandQueue) and queue.profile
        fn, data = transposes(context, queue)
        begin = time.perf_counter()
        queue.start_tuning()
        for _ in range(20):
            fn()
        elapsed = queue.stop_tuning()
        wall = time.perf_counter() - begin
        print(f"tuning queue: {elapsed * 1e6:.1f} us on the device, {wall * 1e6:.1f} us on the host")
        assert isinstance(elapsed, float)
        assert 0 < elapsed <= wall
        with pytest.raises(AssertionError):
            queue.stop_tuning()
        np.testing.assert_array_equal(fn.buffer("dest").get(queue), data.T)


# ------------------------------------------------- borrowed stream and zero-copy views
class TestTorch:
    @pytest.fixture
    def torch(self):
        return pytest.importorskip("torch")

    @pytest.fixture
    def borrowed(self, torch, context):
        from katsdpsigproc_amd import hip

        return hip.CommandQueue(context, stream=torch.cuda.current_stream().cuda_stream)

    def test_a_borrowed_stream_is_not_destroyed(self, torch, context):
        from katsdpsigproc_amd import accel, hip

        stream = torch.cuda.current_stream()
        queue = hip.CommandQueue(context, stream=stream.cuda_stream)
        assert queue.stream == stream.cuda_stream
        assert not hasattr(queue, "_finalizer")
        assert hasattr(context.create_command_queue(), "_finalizer")
        array = accel.DeviceArray(context, (4, 5), np.float32, (4, 8))
        data = it.values((4, 5), np.float32, seed=12)
        array.set(queue, data)
        del queue
        gc.collect()
        tensor = torch.as_tensor(array.buffer, device="cuda")
        doubled = (tensor * 2).cpu().numpy()
        stream.synchronize()
        np.testing.assert_array_equal(doubled[:, :5], data * 2)
        assert torch.cuda.current_stream().cuda_stream == stream.cuda_stream

    @pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.complex64])
    def test_tensor_views_share_the_memory(self, dtype, torch, context, borrowed):
        from katsdpsigproc_amd import accel

        array = accel.DeviceArray(context, (6, 10), dtype, (7, 16))
        interface = array.buffer.__cuda_array_interface__
        assert interface["shape"] == (7, 16) and interface["typestr"] == np.dtype(dtype).str
        assert interface["data"] == (array.buffer.ptr, False)
        tensor = torch.as_tensor(array.buffer, device="cuda")
        assert tensor.data_ptr() == array.buffer.ptr
        assert tuple(tensor.shape) == (7, 16) and tensor.is_contiguous()
        assert tensor.numpy(force=True).dtype == np.dtype(dtype)
        # written through torch, read by DeviceArray.get
        data = it.values((7, 16), dtype, seed=13)
        tensor.copy_(torch.from_numpy(data))
        torch.cuda.current_stream().synchronize()
        got = array.get(borrowed)
        it.same_bytes(data, accel.HostArray.padded_view(got), "written through torch")
        it.same_bytes(data[:6, :10], np.asarray(got), "window")

    @pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.complex64])
    def test_torch_reads_what_the_borrowed_queue_wrote(self, dtype, torch, context, borrowed):
        from katsdpsigproc_amd import transpose

        fn = transpose.TransposeTemplate(context, dtype, "x").instantiate(borrowed, (53, 81))
        fn.ensure_all_bound()
        data = it.values((53, 81), dtype, seed=14)
        fn.buffer("dest").zero(borrowed)
        fn.buffer("src").set(borrowed, data)
        fn()
        # no finish(): torch's copy runs on the same stream, behind the kernel
        dest = fn.buffer("dest")
        tensor = torch.as_tensor(dest.buffer, device="cuda")
        got = tensor.cpu().numpy()
        assert got.shape == dest.padded_shape
        it.same_bytes(data.T, got[:81, :53], "transpose on the borrowed queue")
        assert not got[:, 53:].view(np.uint8).any() and not got[81:].view(np.uint8).any()
