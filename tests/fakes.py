"""Stand-ins for the HIP backend so that slot wiring and host logic can be tested
without a GPU: buffers are numpy arrays, kernels record their launches."""

import numpy as np

from katsdpsigproc_amd import accel


class FakeBuffer:
    def __init__(self, shape, dtype):
        self.array = np.zeros(shape, dtype)
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = self.array.nbytes
        self.ptr = self.array.ctypes.data


class FakeKernel:
    def __init__(self, name):
        self.name = name


class FakeDevice:
    name = "fake"
    platform_name = "fake platform"
    driver_version = "0"
    simd_group_size = 64


class FakeContext:
    def __init__(self):
        self.device = FakeDevice()
        self.raw_allocations = []

    def native_kernel(self, name):
        return FakeKernel(name)

    def allocate_raw(self, n_bytes):
        raw = np.zeros(n_bytes, np.uint8)
        self.raw_allocations.append(raw)
        return raw

    def allocate(self, shape, dtype, raw=None):
        return FakeBuffer(shape, dtype)

    def allocate_pinned(self, shape, dtype):
        return np.empty(shape, dtype)

    def create_command_queue(self, profile=False):
        return FakeQueue(self)


class FakeQueue:
    def __init__(self, context):
        self.context = context
        self.launches = []

    def enqueue_kernel(self, kernel, args, global_size=None, local_size=None):
        self.launches.append((kernel.name, list(args)))

    def enqueue_write_buffer(self, buffer, data, blocking=True):
        buffer.array[...] = data

    def enqueue_read_buffer(self, buffer, data, blocking=True):
        data[...] = buffer.array

    def enqueue_zero_buffer(self, buffer):
        buffer.array[...] = 0

    # -- rectangular copies: byte origins, a shape whose element 0 is a byte count and byte
    # strides, innermost first (the calling convention of AbstractCommandQueue)
    @staticmethod
    def _rect_view(storage, origin, shape, strides):
        """The bytes that (origin, shape, strides) select from `storage` (a FakeBuffer or a
        contiguous host array), as a strided view with the outermost axis first."""
        if not 1 <= len(shape) <= 3 or len(strides) != len(shape):
            raise ValueError("rect copies support 1 to 3 dimensions")
        array = storage.array if isinstance(storage, FakeBuffer) else storage
        assert array.flags.c_contiguous
        flat = array.reshape(-1).view(np.uint8)
        assert np.shares_memory(flat, array)
        assert all(n > 0 for n in shape) and origin >= 0
        last = origin + sum((n - 1) * s for n, s in zip(shape, strides))
        if last >= flat.size:
            raise IndexError(f"rect copy reaches byte {last} of a buffer of {flat.size}")
        return np.lib.stride_tricks.as_strided(
            flat[origin:], tuple(reversed(shape)), tuple(reversed(strides)))  # fmt: skip

    def enqueue_copy_buffer_rect(
        self, src_buffer, dest_buffer, src_origin, dest_origin, shape, src_strides, dest_strides
    ):
        src = self._rect_view(src_buffer, src_origin, shape, src_strides)
        self._rect_view(dest_buffer, dest_origin, shape, dest_strides)[...] = src

    def enqueue_read_buffer_rect(
        self, buffer, data, buffer_origin, data_origin, shape, buffer_strides, data_strides,
        blocking=True,
    ):  # fmt: skip
        src = self._rect_view(buffer, buffer_origin, shape, buffer_strides)
        self._rect_view(data, data_origin, shape, data_strides)[...] = src

    def enqueue_write_buffer_rect(
        self, buffer, data, buffer_origin, data_origin, shape, buffer_strides, data_strides,
        blocking=True,
    ):  # fmt: skip
        src = self._rect_view(data, data_origin, shape, data_strides)
        self._rect_view(buffer, buffer_origin, shape, buffer_strides)[...] = src

    def finish(self):
        pass


def make_queue():
    return FakeContext().create_command_queue()
