"""Two-dimensional (time x frequency) SumThreshold flagger on the GPU.

Drop-in for ``katsdpsigproc.rfi.twodflag.SumThresholdFlagger`` (reference
rfi/twodflag.py:495-720): the same constructor, attributes and ``get_flags``, bit-identical
flags (see DESIGN.md section 9 for the arithmetic followed), computed by the HIP kernels of
``csrc/twodflag.hip``. :class:`SumThresholdFlaggerDeviceTemplate` is the device
:class:`~katsdpsigproc_amd.accel.Operation` behind it, for pipelines that keep the block on
the device.

:func:`masked_gaussian_filter` is the module's other public name (reference
rfi/twodflag.py:360-400), bit-identical as well, on the kernels of ``csrc/masked_filter.hip``;
:class:`MaskedGaussianFilterTemplate` is its device operation.
"""

import ctypes
import math
from typing import Any, Mapping, Optional, Sequence, Tuple

import numpy as np

from .. import _lib, _native_op, accel
from ..abc import AbstractCommandQueue, AbstractContext

#: reference rfi/__init__.py
MAD_NORMAL = 1.4826
MAX_TIME = 4096
MAX_CHANNELS = 65536
MAX_WINDOWS = _lib.TDF_MAX_WINDOWS
MAX_CHUNKS = _lib.TDF_MAX_CHUNKS
MAX_ITERATIONS = 64
#: device workspace per batch of baselines, unless a batch size is given
DEFAULT_WORKSPACE_BYTES = 2 << 30
#: limits of the masked Gaussian filter
MAX_FILTER_DIM = 65536
MAX_FILTER_PASSES = 8
MAX_FILTER_RADIUS = 2047


def _as_min_dtype(value):
    """The reference's narrowest unsigned 0-d array for a non-negative integer."""
    for dtype, limit in ((np.uint8, 2**8), (np.uint16, 2**16), (np.uint32, 2**32)):
        if 0 <= value < limit:
            return np.array(value, dtype)
    return np.array(value, np.int64)


class _Conditioned:
    """Constructor conditioning of the reference (``__init__``), shared by both classes."""

    def _condition(self, outlier_nsigma, windows_time, windows_freq, background_reject,
                   background_iterations, spike_width_time, spike_width_freq, time_extend,
                   freq_extend, freq_chunks, average_freq, flag_all_time_frac,
                   flag_all_freq_frac, rho) -> None:  # fmt: skip
        self.outlier_nsigma = outlier_nsigma
        self.windows_time = windows_time
        windows_freq = np.ceil(np.array(windows_freq, dtype=np.float32) / average_freq)
        self.windows_freq = np.unique(windows_freq.astype(np.int_))
        self.background_reject = background_reject
        self.background_iterations = background_iterations
        self.spike_width_time = spike_width_time
        self.spike_width_freq = spike_width_freq / average_freq
        self.time_extend = _as_min_dtype(time_extend)
        self.freq_extend = _as_min_dtype(freq_extend)
        self.freq_chunks = freq_chunks
        self.average_freq = _as_min_dtype(average_freq)
        self.flag_all_time_frac = flag_all_time_frac
        self.flag_all_freq_frac = flag_all_freq_frac
        self.rho = rho

    def _check_config(self) -> None:
        if not 1 <= int(self.average_freq) <= 1 << 20:
            raise ValueError("average_freq must be in 1..1048576")
        if not 1 <= self.freq_chunks <= MAX_CHUNKS:
            raise ValueError(f"freq_chunks must be in 1..{MAX_CHUNKS}")
        if not 0 <= self.background_iterations <= MAX_ITERATIONS:
            raise ValueError(f"background_iterations must be in 0..{MAX_ITERATIONS}")
        if len(self.windows_time) > MAX_WINDOWS or len(self.windows_freq) > MAX_WINDOWS:
            raise ValueError(f"at most {MAX_WINDOWS} windows per axis are supported")
        it = max(self.background_iterations, 1)
        if not (0 <= self.spike_width_time * it < 4000 and 0 <= self.spike_width_freq * it < 4000):
            raise ValueError("spike_width x background_iterations must be in 0..4000 "
                             "(box-filter radius up to 2047)")  # fmt: skip
        for name in ("time_extend", "freq_extend"):
            if not 0 <= int(getattr(self, name)) <= 1 << 30:
                raise ValueError(f"{name} must be in 0..2**30")

    def _params(self, n_time: int, n_freq: int, is_amplitude: bool) -> _lib.TwodflagParams:
        """What the reference's ``_get_flags`` hands to ``_get_flags_impl`` for this shape."""
        if not 1 <= n_time <= MAX_TIME:
            raise ValueError(f"n_time must be in 1..{MAX_TIME}")
        if not 1 <= n_freq <= MAX_CHANNELS:
            raise ValueError(f"the number of channels must be in 1..{MAX_CHANNELS}")
        average_freq = int(self.average_freq)
        averaged_channels = (n_freq + average_freq - 1) // average_freq
        freq_chunk_ends = np.linspace(0, averaged_channels, self.freq_chunks + 1).astype(np.int_)
        # the reference clips the time windows against the channel count (sic)
        windows_time = np.array([w for w in self.windows_time if w <= n_freq], np.int_)
        windows_freq = np.array([w for w in self.windows_freq if w <= averaged_channels], np.int_)
        if windows_time.size == 0 or windows_freq.size == 0:
            # the reference fails in np.max(windows) the same way
            raise ValueError("zero-size array to reduction operation maximum which has no identity")
        if np.any(windows_time < 1) or np.any(windows_time > 1 << 20):
            raise ValueError("windows_time must be in 1..1048576")
        p = _lib.TwodflagParams()
        p.n_time, p.n_freq, p.average_freq = n_time, n_freq, average_freq
        p.is_amplitude = int(bool(is_amplitude))
        p.n_windows_time, p.n_windows_freq = windows_time.size, windows_freq.size
        for i, w in enumerate(windows_time):
            p.windows_time[i] = int(w)
            p.tf_time[i] = float(pow(self.rho, np.log2(w)))
        for i, w in enumerate(windows_freq):
            p.windows_freq[i] = int(w)
            p.tf_freq[i] = float(pow(self.rho, np.log2(w)))
        p.n_chunks = self.freq_chunks
        for i, e in enumerate(freq_chunk_ends):
            p.chunk_ends[i] = int(e)
        p.background_iterations = self.background_iterations
        p.time_extend, p.freq_extend = int(self.time_extend), int(self.freq_extend)
        p.spike_width_time = float(self.spike_width_time)
        p.spike_width_freq = float(self.spike_width_freq)
        p.threshold_scale = float(self.outlier_nsigma * MAD_NORMAL)
        p.reject_scale = float(MAD_NORMAL * self.background_reject)
        p.flag_all_time_frac = float(self.flag_all_time_frac)
        p.flag_all_freq_frac = float(self.flag_all_freq_frac)
        return p


class SumThresholdFlaggerDeviceTemplate(_Conditioned):
    """Device form of the reference's ``SumThresholdFlagger``.

    Takes the reference constructor's keywords (same defaults) plus `amplitudes`: True for
    float32 magnitudes in, False for complex64 visibilities.
    """

    def __init__(self, context: AbstractContext, outlier_nsigma=4.5, windows_time=[1, 2, 4, 8],
                 windows_freq=[1, 2, 4, 8], background_reject=2.0, background_iterations=1,
                 spike_width_time=12.5, spike_width_freq=10.0, time_extend=3, freq_extend=3,
                 freq_chunks=10, average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8,
                 rho=1.3, amplitudes: bool = False) -> None:  # fmt: skip
        self._condition(outlier_nsigma, windows_time, windows_freq, background_reject,
                        background_iterations, spike_width_time, spike_width_freq, time_extend,
                        freq_extend, freq_chunks, average_freq, flag_all_time_frac,
                        flag_all_freq_frac, rho)  # fmt: skip
        self._check_config()
        self.context = context
        self.amplitudes = bool(amplitudes)
        self.kernel = context.native_kernel("ksp_twodflag")

    def instantiate(self, command_queue: AbstractCommandQueue, n_time: int, n_freq: int,
                    n_baselines: int, batch: Optional[int] = None,
                    allocator: Optional[accel.AbstractAllocator] = None
                    ) -> "SumThresholdFlaggerDevice":  # fmt: skip
        return SumThresholdFlaggerDevice(self, command_queue, n_time, n_freq, n_baselines, batch,
                                         allocator)  # fmt: skip


class SumThresholdFlaggerDevice(accel.Operation):
    """Concrete :class:`SumThresholdFlaggerDeviceTemplate`.

    .. rubric:: Slots

    **data** : time x frequency x baseline, complex64 (float32 with ``amplitudes``)
    **input_flags** : time x frequency x baseline, uint8 (non-zero = flagged)
    **flags** : time x frequency x baseline, uint8 (1 = flagged)

    The three slots share their dimensions (and so their padding). Baselines are processed
    in batches of `batch` (by default as many as fit :data:`DEFAULT_WORKSPACE_BYTES` of
    workspace); the workspace is allocated once, here.
    """

    def __init__(self, template: SumThresholdFlaggerDeviceTemplate,
                 command_queue: AbstractCommandQueue, n_time: int, n_freq: int,
                 n_baselines: int, batch: Optional[int] = None,
                 allocator: Optional[accel.AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(command_queue, allocator)
        if n_baselines < 1:
            raise ValueError("n_baselines must be at least 1")
        self.template = template
        self.shape = (n_time, n_freq, n_baselines)
        self.params = template._params(n_time, n_freq, template.amplitudes)
        size = ctypes.c_size_t()
        _lib.call("ksp_twodflag_workspace", ctypes.byref(self.params), 1, ctypes.byref(size))
        if batch is None:
            batch = max(1, DEFAULT_WORKSPACE_BYTES // size.value)
        self.batch = max(1, min(int(batch), n_baselines))
        _lib.call("ksp_twodflag_workspace", ctypes.byref(self.params), self.batch,
                  ctypes.byref(size))  # fmt: skip
        self.workspace_bytes = size.value
        self.workspace = accel.DeviceArray(command_queue.context, (size.value,), np.uint8)
        dims = (accel.Dimension(n_time), accel.Dimension(n_freq), accel.Dimension(n_baselines))
        dtype = np.float32 if template.amplitudes else np.complex64
        self.slots["data"] = accel.IOSlot(dims, dtype)
        self.slots["input_flags"] = accel.IOSlot(dims, np.uint8)
        self.slots["flags"] = accel.IOSlot(dims, np.uint8)

    def _run(self) -> None:
        data = self.buffer("data")
        in_flags = self.buffer("input_flags")
        out = self.buffer("flags")
        padded = data.padded_shape
        if in_flags.padded_shape != padded or out.padded_shape != padded:
            raise ValueError("data, input_flags and flags must have the same padding")
        n_bl = self.shape[2]
        for bl0 in range(0, n_bl, self.batch):
            self.command_queue.enqueue_kernel(
                self.template.kernel,
                [
                    data.buffer, in_flags.buffer, out.buffer, n_bl,
                    padded[1] * padded[2], padded[2], bl0, min(self.batch, n_bl - bl0),
                    ctypes.byref(self.params), self.workspace.buffer, self.workspace_bytes,
                ],
            )  # fmt: skip

    def parameters(self) -> Mapping[str, Any]:
        t = self.template
        return {
            "shape": self.shape, "batch": self.batch, "amplitudes": t.amplitudes,
            "outlier_nsigma": t.outlier_nsigma, "windows_time": list(t.windows_time),
            "windows_freq": list(t.windows_freq), "background_reject": t.background_reject,
            "background_iterations": t.background_iterations,
            "spike_width_time": t.spike_width_time, "spike_width_freq": t.spike_width_freq,
            "time_extend": int(t.time_extend), "freq_extend": int(t.freq_extend),
            "freq_chunks": t.freq_chunks, "average_freq": int(t.average_freq),
            "flag_all_time_frac": t.flag_all_time_frac,
            "flag_all_freq_frac": t.flag_all_freq_frac, "rho": t.rho,
        }  # fmt: skip


class SumThresholdFlagger(_Conditioned):
    """The reference's ``SumThresholdFlagger`` (same constructor and attributes), run on
    the GPU. ``get_flags`` returns ``np.bool_`` flags bit-identical to the reference's."""

    def __init__(self, outlier_nsigma=4.5, windows_time=[1, 2, 4, 8], windows_freq=[1, 2, 4, 8],
                 background_reject=2.0, background_iterations=1, spike_width_time=12.5,
                 spike_width_freq=10.0, time_extend=3, freq_extend=3, freq_chunks=10,
                 average_freq=1, flag_all_time_frac=0.6, flag_all_freq_frac=0.8, rho=1.3,
                 context: Optional[AbstractContext] = None) -> None:  # fmt: skip
        self._condition(outlier_nsigma, windows_time, windows_freq, background_reject,
                        background_iterations, spike_width_time, spike_width_freq, time_extend,
                        freq_extend, freq_chunks, average_freq, flag_all_time_frac,
                        flag_all_freq_frac, rho)  # fmt: skip
        self._check_config()
        self._context = context
        self._queue = None

    def _device_template(self, amplitudes: bool) -> SumThresholdFlaggerDeviceTemplate:
        if self._context is None:
            self._context = accel.create_some_context(interactive=False)
        if self._queue is None:
            self._queue = self._context.create_command_queue()
        template = SumThresholdFlaggerDeviceTemplate.__new__(SumThresholdFlaggerDeviceTemplate)
        template.__dict__.update({k: v for k, v in self.__dict__.items() if not k.startswith("_")})
        template.context = self._context
        template.amplitudes = amplitudes
        template.kernel = self._context.native_kernel("ksp_twodflag")
        return template

    def get_flags(self, data, flags, pool=None, chunk_size=None, is_multiprocess=None):
        """Flags for `data` (time, frequency, baseline), complex64 or float32 magnitudes,
        with input `flags` of the same shape (non-zero = flagged). `pool` and
        `is_multiprocess` are accepted for compatibility; `chunk_size` bounds the
        baselines per device batch. Neither input is modified."""
        if data.shape != flags.shape:
            raise ValueError("Shape mismatch")
        if data.ndim != 3:
            raise ValueError("data has wrong number of dimensions")
        if data.dtype == np.complex64:
            amplitudes = False
        elif data.dtype == np.float32:
            amplitudes = True
        else:
            raise TypeError(f"data must be complex64 or float32, not {data.dtype}")
        n_time, n_freq, n_bl = data.shape
        if n_bl == 0:
            return np.zeros(data.shape, np.bool_)
        template = self._device_template(amplitudes)
        op = template.instantiate(self._queue, n_time, n_freq, n_bl, batch=chunk_size or None)
        inputs = {"data": np.ascontiguousarray(data),
                  "input_flags": np.ascontiguousarray(flags != 0).view(np.uint8)}  # fmt: skip
        return _native_op.run_once(op, self._queue, inputs, ["flags"])[0].view(np.bool_)


def _filter_radius(sigma: float, passes: int) -> int:
    """Box radius for `sigma` (reference ``_box_gaussian_filter``), in float64."""
    return int(0.5 * math.sqrt(12.0 * float(sigma) ** 2 / passes + 1))


def _filter_divisor(radius: int, passes: int, dtype) -> float:
    """``dtype(2 * radius + 1) ** passes`` as numba computes it (``int_power_impl``): by
    squaring and multiplying, every product rounded to `dtype`."""
    scalar = np.dtype(dtype).type
    result, base, e = scalar(1), scalar(2 * radius + 1), int(passes)
    with np.errstate(over="ignore"):  # (the last squaring is not used)
        while e:
            if e & 1:
                result = scalar(result * base)
            base = scalar(base * base)
            e >>= 1
    return float(result)


def _check_passes(passes) -> None:
    if isinstance(passes, (bool, np.bool_)) or not isinstance(passes, (int, np.integer)):
        raise TypeError("passes must be an integer")
    if not 1 <= passes <= MAX_FILTER_PASSES:
        raise ValueError(f"passes must be in 1..{MAX_FILTER_PASSES}")


def _filter_radii(rows: int, cols: int, sigma, passes: int):
    """Checks the image shape and `sigma` against the limits; returns (sigma, radii)."""
    if not (1 <= rows <= MAX_FILTER_DIM and 1 <= cols <= MAX_FILTER_DIM):
        raise ValueError(f"rows and cols must be in 1..{MAX_FILTER_DIM}")
    sigma = tuple(float(s) for s in sigma)
    if len(sigma) != 2:
        raise ValueError("sigma has wrong number of elements")
    if not all(math.isfinite(s) for s in sigma):
        raise ValueError("sigma must be finite")
    radii = tuple(_filter_radius(s, passes) for s in sigma)
    if max(radii) > MAX_FILTER_RADIUS:
        raise ValueError(f"sigma gives a box radius outside 0..{MAX_FILTER_RADIUS}")
    if passes == 1 and (radii[0] > rows or radii[1] > cols):
        # (the reference indexes before the start of its padded line there)
        raise ValueError("with passes = 1 the box radius must be in 0..the length of its axis")
    return sigma, radii


class MaskedGaussianFilterTemplate:
    """Device form of the reference's ``masked_gaussian_filter`` for images of `dtype`
    (float32 or float64), with `passes` box passes (1..8) per filtered axis."""

    def __init__(self, context: AbstractContext, dtype=np.float32, passes: int = 4) -> None:
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"dtype must be float32 or float64, not {dtype}")
        _check_passes(passes)
        self.context = context
        self.dtype = dtype
        self.passes = int(passes)
        self.kernel = context.native_kernel("ksp_masked_filter")

    def instantiate(self, command_queue: AbstractCommandQueue, shape: Sequence[int],
                    sigma: Sequence[float], batch: Optional[int] = None,
                    allocator: Optional[accel.AbstractAllocator] = None
                    ) -> "MaskedGaussianFilter":  # fmt: skip
        return MaskedGaussianFilter(self, command_queue, shape, sigma, batch, allocator)


class MaskedGaussianFilter(accel.Operation):
    """Concrete :class:`MaskedGaussianFilterTemplate` for images of `shape`, ``(rows,
    cols)`` or ``(images, rows, cols)``, and a pair `sigma` (axis 0, axis 1).

    .. rubric:: Slots

    **data** : shape, `dtype`
    **flags** : shape, uint8 (non-zero = flagged, ignored by the filter)
    **out** : shape, `dtype`; NaN where the filter's support holds no unflagged sample

    The three slots share their dimensions (and so their padding). `out` may be bound to
    the buffer of `data`: the input is read into the workspace before any result of the
    same batch of images is written. Images are processed in batches of `batch` (by
    default as many as fit :data:`DEFAULT_WORKSPACE_BYTES` of workspace, at least one); the
    workspace is allocated once, here.
    """

    def __init__(self, template: MaskedGaussianFilterTemplate,
                 command_queue: AbstractCommandQueue, shape: Sequence[int],
                 sigma: Sequence[float], batch: Optional[int] = None,
                 allocator: Optional[accel.AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(command_queue, allocator)
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (2, 3):
            raise ValueError("shape must be (rows, cols) or (images, rows, cols)")
        images, rows, cols = (1,) + shape if len(shape) == 2 else shape
        if images < 1:
            raise ValueError("the number of images must be at least 1")
        passes = template.passes
        sigma, radii = _filter_radii(rows, cols, sigma, passes)
        self.template = template
        self.shape = shape
        self.images, self.rows, self.cols = images, rows, cols
        self.sigma = sigma
        self.radii = radii
        self.divisors = tuple(_filter_divisor(r, passes, template.dtype) for r in radii)
        itemsize = template.dtype.itemsize
        size = ctypes.c_size_t()
        _lib.call("ksp_masked_filter_workspace", rows, cols, 1, radii[0], radii[1], passes,
                  itemsize, ctypes.byref(size))  # fmt: skip
        if batch is None:
            batch = max(1, DEFAULT_WORKSPACE_BYTES // size.value)
        self.batch = max(1, min(int(batch), images))
        _lib.call("ksp_masked_filter_workspace", rows, cols, self.batch, radii[0], radii[1],
                  passes, itemsize, ctypes.byref(size))  # fmt: skip
        self.workspace_bytes = size.value
        self.workspace = accel.DeviceArray(command_queue.context, (size.value,), np.uint8)
        dims = tuple(accel.Dimension(s) for s in shape)
        self.slots["data"] = accel.IOSlot(dims, template.dtype)
        self.slots["flags"] = accel.IOSlot(dims, np.uint8)
        self.slots["out"] = accel.IOSlot(dims, template.dtype)

    def _run(self) -> None:
        data = self.buffer("data")
        flags = self.buffer("flags")
        out = self.buffer("out")
        padded = data.padded_shape
        if flags.padded_shape != padded or out.padded_shape != padded:
            raise ValueError("data, flags and out must have the same padding")
        row_stride = padded[-1]
        image_stride = padded[-2] * padded[-1]
        for image0 in range(0, self.images, self.batch):
            self.command_queue.enqueue_kernel(
                self.template.kernel,
                [
                    data.buffer, flags.buffer, out.buffer, self.rows, self.cols, self.images,
                    image_stride, row_stride, image0, min(self.batch, self.images - image0),
                    self.radii[0], self.radii[1], self.template.passes, self.divisors[0],
                    self.divisors[1], self.template.dtype.itemsize, self.workspace.buffer,
                    self.workspace_bytes,
                ],
            )  # fmt: skip

    def parameters(self) -> Mapping[str, Any]:
        return {
            "shape": self.shape, "dtype": self.template.dtype.name,
            "passes": self.template.passes, "sigma": self.sigma, "radii": self.radii,
            "batch": self.batch,
        }  # fmt: skip


_filter_context: Optional[AbstractContext] = None
_filter_default_queue: Any = None


def _filter_queue(context: Optional[AbstractContext]) -> Tuple[AbstractContext, Any]:
    """The context and a queue of it: the caller's context with a queue of its own for this
    call (nothing of it is kept), or the module's own pair, created on first use and kept."""
    global _filter_context, _filter_default_queue
    if context is not None:
        return context, context.create_command_queue()
    if _filter_context is None:
        _filter_context = accel.create_some_context(interactive=False)
        _filter_default_queue = _filter_context.create_command_queue()
    return _filter_context, _filter_default_queue


def masked_gaussian_filter(data, flags, sigma, out, passes=4, *, context=None):
    """The reference's ``masked_gaussian_filter``, run on the GPU: fills `out` with the
    approximate Gaussian filter of the 2-D image `data` (float32 or float64) that ignores
    the samples whose `flags` (bool or integer, non-zero = flagged) are set; NaN where the
    filter's support holds no unflagged sample. `sigma` is a pair (axis 0, axis 1) or one
    value for both. `out` has the dtype and shape of `data` and may be `data` itself;
    `data` and `flags` are otherwise not modified. Returns ``None``. `context` names the
    device context to use (no reference to it is kept); by default one context and queue
    are created on the first call and kept. This is a convenience for arrays on the host:
    every call builds its operation, allocates the device buffers and workspace and copies
    both ways. Code that filters many images of one shape keeps a
    :class:`MaskedGaussianFilter` instead."""
    data_dtype = getattr(data, "dtype", None)
    if data_dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"data must be float32 or float64, not {data_dtype}")
    if not isinstance(out, np.ndarray) or out.dtype != data_dtype:
        raise TypeError(f"out must be a {data_dtype} array, not {getattr(out, 'dtype', type(out))}")
    flags = np.asarray(flags)
    if flags.dtype != np.bool_ and not np.issubdtype(flags.dtype, np.integer):
        raise TypeError(f"flags must be bool or an integer type, not {flags.dtype}")
    if data.shape != flags.shape:
        raise ValueError("shape mismatch between data and flags")
    if data.shape != out.shape:
        raise ValueError("shape mismatch between data and out")
    if data.ndim != 2:
        raise ValueError("data has wrong number of dimensions")
    sigma = np.atleast_1d(np.asarray(sigma, np.float64))
    if sigma.shape == (1,):
        sigma = np.repeat(sigma, 2)
    if sigma.shape != (2,):
        raise ValueError("sigma has wrong number of elements")
    _check_passes(passes)
    if data.size == 0:
        return None  # nothing to fill
    _filter_radii(data.shape[0], data.shape[1], sigma, passes)
    context, queue = _filter_queue(context)
    template = MaskedGaussianFilterTemplate(context, data_dtype, passes)
    op = template.instantiate(queue, data.shape, sigma)
    inputs = {"data": np.ascontiguousarray(data),
              "flags": np.ascontiguousarray(flags != 0).view(np.uint8)}  # fmt: skip
    out[...] = _native_op.run_once(op, queue, inputs, ["out"])[0]
    return None
