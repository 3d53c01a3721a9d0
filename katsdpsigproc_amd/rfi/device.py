"""RFI flagging on MI355X behind the reference's template/operation API.

Class names, constructor and ``instantiate`` signatures, slot names and error
behaviour follow the reference (reference: src/katsdpsigproc/rfi/device.py). What is
underneath is different: every operation launches an ahead-of-time compiled HIP kernel
for gfx950 through the C-ABI (``include/katsdpsigproc_hip.h``), and
:class:`FlaggerDeviceTemplate` can replace the five-kernel sequence by one fused
single-pass kernel (:class:`FusedFlaggerDevice`) that is bit-identical to
:class:`katsdpsigproc_amd.rfi.host.FlaggerHost`.

As in the reference, noise estimators and thresholders may work on transposed
(baseline-major) data, advertised by their ``transposed`` attribute; the flagger
inserts transposes where needed.
"""

import ctypes
from abc import ABC, abstractmethod
from typing import Any, List, Mapping, Optional, Tuple, Type, Union

import numpy as np

from .. import _lib, _native_op, accel, transpose, tune
from ..abc import AbstractCommandQueue, AbstractContext
from ..accel import AbstractAllocator
from . import BackgroundFlags, host

_THRESHOLD_SUM_DEFAULT_THRESHOLD_FALLOFF = 1.2


def ctypes_float_array(values):
    return (ctypes.c_float * len(values))(*[float(v) for v in values])


def ctypes_double_array(values):
    return (ctypes.c_double * len(values))(*[float(v) for v in values])


def _check_shape(channels: int, baselines: int) -> None:
    if channels < 1 or baselines < 1:
        raise ValueError("channels and baselines must be at least 1")


# ----------------------------------------------------------------- abstract interfaces
class AbstractBackgroundDevice(accel.Operation):
    pass


class AbstractBackgroundDeviceTemplate(ABC):
    use_flags: BackgroundFlags
    context: AbstractContext
    host_class: Type[host.AbstractBackgroundHost]

    @abstractmethod
    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    allocator: Optional[AbstractAllocator] = None) -> AbstractBackgroundDevice:  # fmt: skip
        """Create an instance."""


class AbstractNoiseEstDevice(accel.Operation):
    transposed: bool


class AbstractNoiseEstDeviceTemplate(ABC):
    transposed: bool
    context: AbstractContext
    host_class: Type[host.AbstractNoiseEstHost]

    @abstractmethod
    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    allocator: Optional[AbstractAllocator] = None) -> AbstractNoiseEstDevice:  # fmt: skip
        """Create an instance."""


class AbstractThresholdDevice(accel.Operation):
    transposed: bool


class AbstractThresholdDeviceTemplate(ABC):
    transposed: bool
    context: AbstractContext
    host_class: Type[host.AbstractThresholdHost]

    @abstractmethod
    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    n_sigma: float, *,
                    allocator: Optional[AbstractAllocator] = None) -> AbstractThresholdDevice:  # fmt: skip
        """Create an instance (concrete classes may add parameters before `allocator`)."""


# ------------------------------------------------------------------------- background
class BackgroundHostFromDevice(host.AbstractBackgroundHost):
    """Present a device backgrounder template through the host call signature.

    Instantiates, uploads, runs and downloads on every call (reference
    rfi/device.py:113-138). ``TypeError`` if flags are given to a template built without
    them, or omitted from one built with them.
    """

    def __init__(self, template: AbstractBackgroundDeviceTemplate,
                 command_queue: AbstractCommandQueue) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis: np.ndarray, flags: Optional[np.ndarray] = None) -> np.ndarray:
        _native_op.check_optional(flags, self.template.use_flags, "flags")
        channels, baselines = vis.shape
        fn = self.template.instantiate(self.command_queue, channels, baselines)
        inputs = {"vis": vis, "flags": flags}
        return _native_op.run_once(fn, self.command_queue, inputs, ["deviations"])[0]


class BackgroundMedianFilterDeviceTemplate(_native_op.AutotunedTuning,
                                           AbstractBackgroundDeviceTemplate):  # fmt: skip
    """Median-filter backgrounder (reference rfi/device.py:141-262).

    Unlike the reference kernel, which uses ``hypot`` and float32 throughout and so "may
    give slightly different results", this one reproduces the host class: numpy's
    complex64 ``abs``, float64 median and subtraction, result rounded once to float32.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    width
        Window width in channels: odd, 3 to 255 (widths above 31 run a wide-window kernel
        and cannot be fused into :class:`FusedFlaggerDevice`)
    is_amplitude
        Inputs are float32 amplitudes rather than complex64 visibilities
    use_flags
        :class:`BackgroundFlags`, or ``True``/``False`` for CHANNEL/NONE
    tuning
        ``csplit``: into how many channel segments a baseline is cut (each walked by its
        own wavefront, re-reading ``width - 1`` channels of halo); 0 lets the launcher
        choose. ``wgs`` of the reference has no counterpart: a wavefront always covers
        64 adjacent baselines (512-byte coalesced rows). Default: autotuned and cached
        (:mod:`katsdpsigproc_amd.tune`).
    """

    host_class = host.BackgroundMedianFilterHost
    autotune_version = 5
    SUPPORTED_WIDTHS = tuple(range(3, 256, 2))

    def __init__(self, context: AbstractContext, width: int, is_amplitude: bool = False,
                 use_flags: Union[BackgroundFlags, bool] = BackgroundFlags.NONE,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        if use_flags is True:
            use_flags = BackgroundFlags.CHANNEL
        elif use_flags is False:
            use_flags = BackgroundFlags.NONE
        if not isinstance(use_flags, BackgroundFlags):
            raise TypeError("use_flags must be an instance of BackgroundFlags or bool")
        if width not in self.SUPPORTED_WIDTHS:
            raise ValueError(f"width {width} is not an odd number in the range 3..255")
        self.context = context
        self.width = width
        self.is_amplitude = is_amplitude
        self.use_flags = use_flags
        self._init_tuning(tuning, width, is_amplitude, use_flags)
        self.kernel = context.native_kernel("ksp_background_median_filter")

    @classmethod
    @tune.autotuner(test={"wgs": 64, "csplit": 4})
    def autotune(cls, context, width: int, is_amplitude: bool,
                 use_flags: BackgroundFlags) -> Mapping[str, Any]:  # fmt: skip
        """Search ``csplit`` on the reference's tuning shape, 4096 channels x 8192
        baselines (reference rfi/device.py:215-252)."""
        queue = context.create_tuning_command_queue()
        channels, baselines = 4096, 8192
        shape = (channels, baselines)
        vis = accel.DeviceArray(context, shape, np.float32 if is_amplitude else np.complex64)
        deviations = accel.DeviceArray(context, shape, np.float32)
        rs = np.random.RandomState(seed=1)
        if is_amplitude:
            vis.set(queue, np.abs(rs.standard_normal(shape)).astype(np.float32))
        else:
            block = rs.standard_normal(shape + (2,)).astype(np.float32).view(np.complex64)[..., 0]
            vis.set(queue, block)
        flags = None
        if use_flags == BackgroundFlags.CHANNEL:
            flags = accel.DeviceArray(context, (channels,), np.uint8)
            flags.set(queue, (rs.random_sample(channels) < 1 / 16).astype(np.uint8))
        elif use_flags == BackgroundFlags.FULL:
            flags = accel.DeviceArray(context, shape, np.uint8)
            flags.set(queue, (rs.random_sample(shape) < 1 / 16).astype(np.uint8))

        def generate(csplit: int):
            fn = cls(context, width, is_amplitude, use_flags, tuning={"wgs": 64, "csplit": csplit})
            op = fn.instantiate(queue, channels, baselines)
            op.bind(vis=vis, deviations=deviations)
            if flags is not None:
                op.bind(flags=flags)
            return tune.make_measure(queue, op)

        # building a candidate compiles nothing here, so one thread will do
        best = tune.autotune(generate, threads=1, csplit=[0, 8, 16, 32, 64, 128])
        return {"wgs": 64, "csplit": int(best["csplit"])}

    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    allocator: Optional[AbstractAllocator] = None) -> "BackgroundMedianFilterDevice":  # fmt: skip
        return BackgroundMedianFilterDevice(self, command_queue, channels, baselines, allocator)


class BackgroundMedianFilterDevice(_native_op.NativeOperation, AbstractBackgroundDevice):
    """Concrete :class:`BackgroundMedianFilterDeviceTemplate`.

    .. rubric:: Slots

    **vis** : channels x baselines, float32 or complex64
    **flags** : channels x baselines or channels, uint8 (only with ``use_flags``)
    **deviations** : channels x baselines, float32
    """

    def __init__(self, template: BackgroundMedianFilterDeviceTemplate,
                 command_queue: AbstractCommandQueue, channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        vis_type = np.float32 if template.is_amplitude else np.complex64
        # one Dimension object shared by vis, deviations and full flags: equal strides,
        # as in the reference (rfi/device.py:303-307)
        dims = (channels, accel.Dimension(baselines))
        self.slots["vis"] = accel.IOSlot(dims, vis_type)
        self.slots["deviations"] = accel.IOSlot(dims, np.float32)
        if template.use_flags == BackgroundFlags.FULL:
            self.slots["flags"] = accel.IOSlot(dims, np.uint8)
        elif template.use_flags == BackgroundFlags.CHANNEL:
            self.slots["flags"] = accel.IOSlot((channels,), np.uint8)

    def _run(self) -> None:
        vis = self.buffer("vis")
        deviations = self.buffer("deviations")
        mode = self.template.use_flags
        flags = self.buffer("flags") if mode else None
        flags_stride = flags.padded_shape[1] if mode == BackgroundFlags.FULL else 0
        self._launch(
            vis.buffer,
            deviations.buffer,
            _native_op.pointer(flags),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(vis.padded_shape[1]),
            np.int32(flags_stride),
            np.int32(self.template.width),
            np.int32(self.template.is_amplitude),
            np.int32(mode.value),
            np.int32(self.template.tuning.get("csplit", 0)),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            width=self.template.width,
            use_flags=self.template.use_flags.name,
            csplit=self.template.tuning.get("csplit", 0),
        )


# ------------------------------------------------------------------------------ noise
class NoiseEstHostFromDevice(host.AbstractNoiseEstHost):
    """Present a device noise-estimator template through the host call signature."""

    def __init__(self, template: AbstractNoiseEstDeviceTemplate,
                 command_queue: AbstractCommandQueue) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue

    def __call__(self, deviations: np.ndarray) -> np.ndarray:
        channels, baselines = deviations.shape
        fn = self.template.instantiate(self.command_queue, channels, baselines)
        if self.template.transposed:
            deviations = deviations.T
        return _native_op.run_once(fn, self.command_queue, {"deviations": deviations}, ["noise"])[0]


class NoiseEstMADDeviceTemplate(_native_op.AutotunedTuning, AbstractNoiseEstDeviceTemplate):
    """Median of non-zero absolute deviations on channel-major data
    (reference rfi/device.py:363-409). :class:`NoiseEstMADTDeviceTemplate` is faster, as
    the reference also notes (rfi/device.py:366).

    `tuning`: ``method`` -- 0: the direct kernel (strips of 8 baselines through LDS up to
    4096 channels; a column re-read per search pass beyond, as the reference does); 1:
    transpose into a temporary ``deviations_t`` slot, then the baseline-major kernel
    (one more pass over the data, but both passes are coalesced). Default: autotuned and
    cached. ``wgsx``/``wgsy`` of the reference have no counterpart.
    """

    host_class = host.NoiseEstMADHost
    transposed = False
    autotune_version = 2

    def __init__(self, context: AbstractContext,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.context = context
        self._init_tuning(tuning)
        self.kernel = context.native_kernel("ksp_madnz")
        self.kernel_t = context.native_kernel("ksp_madnz_t")
        self.kernel_transpose = context.native_kernel("ksp_transpose")

    @classmethod
    @tune.autotuner(test={"method": 0})
    def autotune(cls, context: AbstractContext) -> Mapping[str, Any]:
        queue = context.create_tuning_command_queue()
        channels, baselines = 4096, 8192
        rs = np.random.RandomState(seed=1)
        data = rs.standard_normal((channels, baselines)).astype(np.float32)

        def generate(method: int):
            op = cls(context, tuning={"method": method}).instantiate(queue, channels, baselines)
            op.ensure_all_bound()
            op.buffer("deviations").set(queue, data)
            return tune.make_measure(queue, op)

        return {"method": int(tune.autotune(generate, threads=1, method=[0, 1])["method"])}

    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    allocator: Optional[AbstractAllocator] = None) -> "NoiseEstMADDevice":  # fmt: skip
        return NoiseEstMADDevice(self, command_queue, channels, baselines, allocator)


class NoiseEstMADDevice(_native_op.NativeOperation, AbstractNoiseEstDevice):
    """Concrete :class:`NoiseEstMADDeviceTemplate`.

    .. rubric:: Slots

    **deviations** : channels x baselines, float32
    **noise** : baselines, float32

    .. rubric:: Temporary slots

    **deviations_t** : baselines x channels, float32 (only with ``method`` 1)
    """

    transposed = False
    #: Longest band for which ``method`` 1 (transpose + the baseline-major kernel) is used;
    #: longer bands take the direct kernel whatever the tuning says.
    MAX_TRANSPOSED_CHANNELS = 256 * 64

    def __init__(self, template: NoiseEstMADDeviceTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        self.method = int(template.tuning.get("method", 0))
        if channels > self.MAX_TRANSPOSED_CHANNELS:
            self.method = 0
        baselines_dim = accel.Dimension(baselines)
        self.slots["noise"] = accel.IOSlot((baselines_dim,), np.float32)
        self.slots["deviations"] = accel.IOSlot((channels, baselines_dim), np.float32)
        if self.method == 1:
            self.slots["deviations_t"] = accel.IOSlot((baselines, accel.Dimension(channels)), np.float32)

    def _run(self) -> None:
        deviations = self.buffer("deviations")
        noise = self.buffer("noise")
        if self.method == 1:
            dev_t = self.buffer("deviations_t")
            self.command_queue.enqueue_kernel(
                self.template.kernel_transpose,
                [
                    dev_t.buffer,
                    deviations.buffer,
                    np.int32(self.channels),
                    np.int32(self.baselines),
                    np.int32(dev_t.padded_shape[1]),
                    np.int32(deviations.padded_shape[1]),
                    np.int32(4),
                ],
            )
            self.command_queue.enqueue_kernel(
                self.template.kernel_t,
                [
                    dev_t.buffer,
                    noise.buffer,
                    np.int32(self.channels),
                    np.int32(self.baselines),
                    np.int32(dev_t.padded_shape[1]),
                ],
            )
            return
        self._launch(
            deviations.buffer,
            noise.buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(deviations.padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(method=self.method)


class NoiseEstMADTDeviceTemplate(_native_op.NativeTemplate, AbstractNoiseEstDeviceTemplate):
    """Median of non-zero absolute deviations on baseline-major data
    (reference rfi/device.py:475-549).

    Parameters
    ----------
    context
        Context whose device will run the kernel
    max_channels
        Upper bound on channels per instance (at most 262144, the reference's bound of
        1024 x 256). Up to 16384 channels a baseline is held in the registers of a
        wavefront or of one 256-work-item workgroup; longer rows go to a 1024-work-item
        workgroup per baseline that selects the median by three histogram passes
    tuning
        The kernel's geometry is fixed (one wavefront or workgroup per baseline):
        ``wgsx`` of the reference is accepted without effect, any other key is a ``ValueError``
        (:func:`.tune.fixed_geometry`).
    """

    host_class = host.NoiseEstMADHost
    transposed = True
    MAX_CHANNELS_SUPPORTED = 256 * 1024
    KERNEL = "ksp_madnz_t"
    TUNING_KEYS = ("wgsx",)

    def __init__(self, context: AbstractContext, max_channels: int,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        if max_channels > self.MAX_CHANNELS_SUPPORTED:
            raise ValueError(f"max_channels exceeds {self.MAX_CHANNELS_SUPPORTED}")
        self.max_channels = max_channels
        self._setup(context, tuning)


class NoiseEstMADTDevice(_native_op.NativeOperation, AbstractNoiseEstDevice):
    """Concrete :class:`NoiseEstMADTDeviceTemplate` (``ValueError`` if `channels` exceeds
    the template's ``max_channels``).

    .. rubric:: Slots

    **deviations** : baselines x channels, float32
    **noise** : baselines, float32
    """

    transposed = True

    def __init__(self, template: NoiseEstMADTDeviceTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels > template.max_channels:
            raise ValueError("channels exceeds max_channels")
        self.slots["noise"] = accel.IOSlot((baselines,), np.float32)
        self.slots["deviations"] = accel.IOSlot((baselines, channels), np.float32)

    def _run(self) -> None:
        deviations = self.buffer("deviations")
        self._launch(
            deviations.buffer,
            self.buffer("noise").buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(deviations.padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(max_channels=self.template.max_channels)


NoiseEstMADTDeviceTemplate.operation_class = NoiseEstMADTDevice


# -------------------------------------------------------------------------- threshold
class ThresholdHostFromDevice(host.AbstractThresholdHost):
    """Present a device thresholder template through the host call signature; extra
    positional/keyword arguments are forwarded to ``instantiate``."""

    def __init__(self, template: AbstractThresholdDeviceTemplate,
                 command_queue: AbstractCommandQueue, *args, **kwargs) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue
        self.args = args
        self.kwargs = kwargs

    def __call__(self, deviations: np.ndarray, noise: np.ndarray) -> np.ndarray:
        channels, baselines = deviations.shape
        fn = self.template.instantiate(
            self.command_queue, channels, baselines, *self.args, **self.kwargs
        )
        transposed = self.template.transposed
        if transposed:
            deviations = deviations.T
        inputs = {"deviations": deviations, "noise": noise}
        flags = _native_op.run_once(fn, self.command_queue, inputs, ["flags"])[0]
        return flags.T if transposed else flags


class ThresholdSimpleDeviceTemplate(_native_op.NativeTemplate, AbstractThresholdDeviceTemplate):
    """Independent per-sample threshold, either memory order
    (reference rfi/device.py:654-720). The kernel's geometry is fixed: ``wgsx``/``wgsy`` of the
    reference are accepted in `tuning` without effect, any other key is a ``ValueError``
    (:func:`.tune.fixed_geometry`)."""

    host_class = host.ThresholdSimpleHost
    KERNEL = "ksp_threshold_simple"
    TUNING_KEYS = ("wgsx", "wgsy")

    def __init__(self, context: AbstractContext, transposed: bool, flag_value: int = 1,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.transposed = transposed
        self.flag_value = flag_value
        self._setup(context, tuning)

    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    n_sigma: float,
                    allocator: Optional[AbstractAllocator] = None) -> "ThresholdSimpleDevice":  # fmt: skip
        return ThresholdSimpleDevice(self, command_queue, channels, baselines, n_sigma, allocator)


class ThresholdSimpleDevice(_native_op.NativeOperation, AbstractThresholdDevice):
    """Concrete :class:`ThresholdSimpleDeviceTemplate`.

    .. rubric:: Slots

    **deviations** : channels x baselines (or transposed), float32
    **noise** : baselines, float32
    **flags** : channels x baselines (or transposed), uint8
    """

    def __init__(self, template: ThresholdSimpleDeviceTemplate,
                 command_queue: AbstractCommandQueue, channels: int, baselines: int,
                 n_sigma: float, allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        self.n_sigma = n_sigma
        self.transposed = template.transposed
        shape = self.layout(self.transposed)
        dims = (accel.Dimension(shape[0]), accel.Dimension(shape[1]))
        noise_dim = dims[0] if self.transposed else dims[1]
        self.slots["deviations"] = accel.IOSlot(dims, np.float32)
        self.slots["noise"] = accel.IOSlot((noise_dim,), np.float32)
        self.slots["flags"] = accel.IOSlot(dims, np.uint8)

    def _run(self) -> None:
        deviations = self.buffer("deviations")
        self._launch(
            deviations.buffer,
            self.buffer("noise").buffer,
            self.buffer("flags").buffer,
            np.int32(deviations.shape[0]),
            np.int32(deviations.shape[1]),
            np.int32(deviations.padded_shape[1]),
            np.float32(self.n_sigma),
            np.int32(self.template.flag_value),
            np.int32(self.transposed),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            n_sigma=self.n_sigma,
            flag_value=self.template.flag_value,
            transposed=self.transposed,
        )


class ThresholdSumDeviceTemplate(_native_op.AutotunedTuning, AbstractThresholdDeviceTemplate):
    """SumThreshold on baseline-major data (reference rfi/device.py:812-907), or on
    channel-major data with ``transposed=False``.

    Follows :class:`host.ThresholdSumHost` exactly (float32 threshold chain, float64
    window sums over full windows only), where the reference kernel uses float32 sums
    and zero-pads the band edges.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    n_windows
        Number of window sizes 1, 2, 4, ... (1 to 8, i.e. windows of up to 128
        channels; the reference sets no limit but its halo, ``2**n - n - 1`` channels
        on each side of a chunk, stops being practical about there)
    flag_value
        Value stored for flagged samples
    tuning
        ``vt``: channels per thread of the 256-thread workgroup (8, 16 or 32, i.e. chunks
        of 2048, 4096 or 8192 channels with a ``2**n_windows - n_windows - 1`` channel
        halo between chunks); 0 lets the launcher choose. ``wgs`` of the reference is
        fixed at 256. Default: autotuned and cached (:mod:`katsdpsigproc_amd.tune`).
        Not used with ``transposed=False``: that launcher picks its own geometry.
    transposed
        ``True`` (default, the reference's only layout): `deviations` and `flags` are
        baselines x channels. ``False``: channels x baselines, the layout the background
        filter writes, so a flagger needs no transposes around this stage (no reference
        counterpart). The flags are the same bit for bit.
    """

    host_class = host.ThresholdSumHost
    transposed = True
    autotune_version = 1

    def __init__(self, context: AbstractContext, n_windows: int = 4, flag_value: int = 1,
                 tuning: Optional[Mapping[str, Any]] = None, *,
                 transposed: bool = True) -> None:  # fmt: skip
        if not 1 <= n_windows <= 8:
            raise ValueError("n_windows must be between 1 and 8")
        self.context = context
        self.n_windows = n_windows
        self.flag_value = flag_value
        self.transposed = bool(transposed)
        if self.transposed:
            self._init_tuning(tuning, n_windows)
            self.kernel = context.native_kernel("ksp_threshold_sum")
        else:
            self._init_tuning({} if tuning is None else tuning)  # nothing to search
            self.kernel = context.native_kernel("ksp_threshold_sum_cm")

    @classmethod
    @tune.autotuner(test={"wgs": 256, "vt": 8})
    def autotune(cls, context: AbstractContext, n_windows: int) -> Mapping[str, Any]:
        """Search ``vt`` on the reference's tuning shape, 4096 channels x 8192 baselines
        with some interference to threshold (reference rfi/device.py:890-907)."""
        queue = context.create_tuning_command_queue()
        channels, baselines = 4096, 8192
        shape = (baselines, channels)
        rs = np.random.RandomState(seed=1)
        dev = rs.standard_normal(shape).astype(np.float32)
        dev[rs.random_sample(shape) < 0.01] += 100.0
        deviations = accel.DeviceArray(context, shape, np.float32)
        deviations.set(queue, dev)
        noise = accel.DeviceArray(context, (baselines,), np.float32)
        noise.set(queue, np.ones(baselines, np.float32))
        flags = accel.DeviceArray(context, shape, np.uint8)

        def generate(vt: int):
            fn = cls(context, n_windows, tuning={"wgs": 256, "vt": vt})
            op = fn.instantiate(queue, channels, baselines, 11.0)
            op.bind(deviations=deviations, noise=noise, flags=flags)
            return tune.make_measure(queue, op)

        best = tune.autotune(generate, threads=1, vt=[8, 16, 32])
        return {"wgs": 256, "vt": int(best["vt"])}

    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    n_sigma: float,
                    threshold_falloff: float = _THRESHOLD_SUM_DEFAULT_THRESHOLD_FALLOFF,
                    allocator: Optional[AbstractAllocator] = None) -> "ThresholdSumDevice":  # fmt: skip
        return ThresholdSumDevice(
            self, command_queue, channels, baselines, n_sigma, threshold_falloff, allocator
        )


class ThresholdSumDevice(_native_op.NativeOperation, AbstractThresholdDevice):
    """Concrete :class:`ThresholdSumDeviceTemplate`.

    .. rubric:: Slots

    **deviations** : baselines x channels (channels x baselines if not transposed), float32
    **noise** : baselines, float32
    **flags** : baselines x channels (channels x baselines if not transposed), uint8
    """

    host_class = host.ThresholdSumHost
    transposed = True
    DEFAULT_THRESHOLD_FALLOFF = _THRESHOLD_SUM_DEFAULT_THRESHOLD_FALLOFF

    def __init__(self, template: ThresholdSumDeviceTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_sigma: float,
                 threshold_falloff: float = DEFAULT_THRESHOLD_FALLOFF,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        self.n_sigma = n_sigma
        self.threshold_falloff = threshold_falloff
        # python-float scales rounded to float32, as numpy does when the host class
        # multiplies a float32 threshold by them (rfi/host.py:215,235)
        self.scales = (ctypes_float_array(
            [np.float32(pow(threshold_falloff, -i)) for i in range(template.n_windows)]
        ))
        self.transposed = template.transposed
        # deviations and flags share the Dimension of the fast axis, hence the stride; channel-
        # major that axis is the baselines and noise shares it too, as in
        # ThresholdSimpleDevice(transposed=False)
        rows, columns = self.layout(self.transposed)
        dims = (rows, accel.Dimension(columns))
        noise_dim = baselines if self.transposed else dims[1]
        self.slots["deviations"] = accel.IOSlot(dims, np.float32)
        self.slots["noise"] = accel.IOSlot((noise_dim,), np.float32)
        self.slots["flags"] = accel.IOSlot(dims, np.uint8)

    def _run(self) -> None:
        deviations = self.buffer("deviations")
        args = [
            deviations.buffer,
            self.buffer("noise").buffer,
            self.buffer("flags").buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(deviations.padded_shape[1]),
            np.float32(self.n_sigma),
            self.scales,
            np.int32(self.template.n_windows),
            np.int32(self.template.flag_value),
        ]
        if self.transposed:  # the channel-major launcher picks its own geometry
            args.append(np.int32(self.template.tuning.get("vt", 0)))
        self._launch(*args)

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            n_sigma=self.n_sigma,
            threshold_falloff=self.threshold_falloff,
            vt=self.template.tuning.get("vt", 0),
            flag_value=self.template.flag_value,
            transposed=self.transposed,
        )


# ---------------------------------------------------------------------------- flagger
class FlaggerDeviceTemplate:
    """Backgrounder + noise estimator + thresholder (reference rfi/device.py:998-1059).

    Parameters
    ----------
    background, noise_est, threshold
        Templates of the three stages (all on one context)
    fused
        ``None`` (default): use the single-pass fused kernel whenever the combination
        and the instantiated shape allow it, otherwise the kernel-per-stage sequence.
        ``True``: require the fused kernel (``ValueError`` at instantiation if it
        cannot be used). ``False``: always build the reference-shaped sequence.
    keep_deviations
        Fused path only: also provide and write the ``deviations`` slot (float32, 4 more
        bytes per sample of HBM traffic). Off by default: in the reference ``deviations``
        is a *temporary* slot of the flagger (reference rfi/device.py:1081-1091), which a
        single-pass kernel has no need to materialise. The sequence always has it.
    tuning
        Fused path only: ``{"vis_pad": n}``, the number of elements by which the rows of the
        ``vis`` slot are padded beyond `baselines` (the kernel reads 32-byte pieces of 4096
        rows at a time, and how fast the memory system serves that depends on the row
        stride: at 32768 baselines 2 % faster with 512, 18 % slower with 256). By default
        it is autotuned per shape when the operation is instantiated.
    """

    autotune_version = 1
    _VIS_PADS = (0, 16, 32, 512, 2048)

    def __init__(self, background: AbstractBackgroundDeviceTemplate,
                 noise_est: AbstractNoiseEstDeviceTemplate,
                 threshold: AbstractThresholdDeviceTemplate,
                 fused: Optional[bool] = None, keep_deviations: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.background = background
        self.noise_est = noise_est
        self.threshold = threshold
        self.fused = fused
        self.keep_deviations = keep_deviations
        self._fused_tuning = dict(tuning) if tuning is not None else None
        context = background.context
        assert noise_est.context is context
        assert threshold.context is context
        self.context = context
        if noise_est.transposed or threshold.transposed:
            self.transpose_deviations: Optional[transpose.TransposeTemplate] = (
                transpose.TransposeTemplate(context, np.float32, "float")
            )
        else:
            self.transpose_deviations = None
        if threshold.transposed:
            self.transpose_flags: Optional[transpose.TransposeTemplate] = (
                transpose.TransposeTemplate(context, np.uint8, "unsigned char")
            )
        else:
            self.transpose_flags = None
        self._fused_kernel = context.native_kernel("ksp_flagger_fused")

    def fusable(self, channels: int) -> bool:
        """Can the fused kernel run this combination of stages at `channels`?"""
        bg, th = self.background, self.threshold
        if not isinstance(bg, BackgroundMedianFilterDeviceTemplate):
            return False
        if not isinstance(self.noise_est, (NoiseEstMADDeviceTemplate, NoiseEstMADTDeviceTemplate)):
            return False
        if isinstance(self.noise_est, NoiseEstMADTDeviceTemplate):
            if channels > self.noise_est.max_channels:
                return False  # keep the error behaviour of the sequence
        if isinstance(th, ThresholdSumDeviceTemplate):
            n_windows = th.n_windows
        elif isinstance(th, ThresholdSimpleDeviceTemplate):
            n_windows = 1
        else:
            return False
        return bool(_lib.call("ksp_flagger_fused_supported", channels, bg.width, n_windows))

    @classmethod
    @tune.autotuner(test={"vis_pad": 0})
    def autotune(cls, context: AbstractContext, channels: int, baselines: int, width: int,
                 is_amplitude: bool, use_flags: BackgroundFlags, sum_threshold: bool,
                 n_windows: int) -> Mapping[str, Any]:  # fmt: skip
        """Row padding of ``vis`` for the fused kernel at exactly this shape: the candidates
        are timed on standard-normal data (no interference, 11 sigma)."""
        if baselines < 2048:
            return {"vis_pad": 0}  # a handful of workgroups per CU: nothing to tune
        queue = context.create_tuning_command_queue()
        rs = np.random.RandomState(seed=1)
        tile = min(baselines, 1024)
        if is_amplitude:
            block = np.abs(rs.standard_normal((channels, tile))).astype(np.float32)
        else:
            block = rs.standard_normal((channels, tile, 2)).astype(np.float32).view(np.complex64)[..., 0]
        data = np.tile(block, (1, -(-baselines // tile)))[:, :baselines]
        if use_flags == BackgroundFlags.CHANNEL:
            mask = (rs.random_sample(channels) < 1 / 16).astype(np.uint8)
        elif use_flags == BackgroundFlags.FULL:
            mask = (rs.random_sample((channels, baselines)) < 1 / 16).astype(np.uint8)
        bg = BackgroundMedianFilterDeviceTemplate(context, width, is_amplitude, use_flags,
                                                  tuning={"wgs": 64, "csplit": 0})  # fmt: skip
        ne = NoiseEstMADTDeviceTemplate(context, max(channels, 1), tuning={"wgsx": 256})
        if sum_threshold:
            th: AbstractThresholdDeviceTemplate = ThresholdSumDeviceTemplate(
                context, n_windows, tuning={"wgsx": 256, "vt": 0})  # fmt: skip
        else:
            th = ThresholdSimpleDeviceTemplate(context, False, tuning={"wgsx": 64, "wgsy": 4})

        def generate(vis_pad: int):
            template = cls(bg, ne, th, fused=True, tuning={"vis_pad": vis_pad})
            op = template.instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
            op.ensure_all_bound()
            op.buffer("vis").set(queue, data)
            if use_flags != BackgroundFlags.NONE:
                op.buffer("input_flags").set(queue, mask)
            for _ in range(60):  # every candidate starts at sustained clocks
                op()
            queue.finish()
            return tune.make_measure(queue, op)

        best = tune.autotune(generate, threads=1, vis_pad=list(cls._VIS_PADS))
        return {"vis_pad": int(best["vis_pad"])}

    def instantiate(self, command_queue: AbstractCommandQueue, channels: int, baselines: int,
                    background_args: Mapping[str, Any] = {},
                    noise_est_args: Mapping[str, Any] = {},
                    threshold_args: Mapping[str, Any] = {},
                    allocator: Optional[AbstractAllocator] = None) -> accel.Operation:  # fmt: skip
        """Create a :class:`FusedFlaggerDevice` or a :class:`FlaggerDevice`."""
        use_fused = self.fused
        if use_fused is None:
            use_fused = (
                self.fusable(channels) and not background_args and not noise_est_args
            )
        elif use_fused and not self.fusable(channels):
            raise ValueError("this combination of stages/shape cannot use the fused kernel")
        if use_fused:
            if self._fused_tuning is not None:
                vis_pad = int(self._fused_tuning.get("vis_pad", 0))
            else:
                th = self.threshold
                vis_pad = int(self.autotune(
                    self.context, channels, baselines, self.background.width,
                    self.background.is_amplitude, self.background.use_flags,
                    isinstance(th, ThresholdSumDeviceTemplate), getattr(th, "n_windows", 1),
                )["vis_pad"])  # fmt: skip
            return FusedFlaggerDevice(
                self, command_queue, channels, baselines, threshold_args, allocator, vis_pad
            )
        return FlaggerDevice(
            self, command_queue, channels, baselines, background_args, noise_est_args,
            threshold_args, allocator,
        )  # fmt: skip


class FlaggerDevice(accel.OperationSequence):
    """The kernel-per-stage flagger, wired exactly as the reference wires it
    (reference rfi/device.py:1062-1166).

    .. rubric:: Slots

    **vis** : channels x baselines, float32 or complex64
    **noise** : baselines, float32
    **flags** : channels x baselines, uint8
    **input_flags** : channels x baselines or channels, uint8 -- only if the backgrounder
        uses flags; they steer the background only, are not copied to the output, and a
        sample flagged here is never flagged as RFI.

    .. rubric:: Temporary slots

    **deviations** : channels x baselines, float32
    **deviations_t** : baselines x channels, float32 (if any stage is transposed)
    **flags_t** : baselines x channels, uint8 (if the thresholder is transposed)
    """

    def __init__(self, template: FlaggerDeviceTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, background_args: Mapping[str, Any] = {},
                 noise_est_args: Mapping[str, Any] = {}, threshold_args: Mapping[str, Any] = {},
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        self.template = template
        self.channels = channels
        self.baselines = baselines
        self.background = template.background.instantiate(
            command_queue, channels, baselines, allocator=allocator, **background_args
        )
        self.noise_est = template.noise_est.instantiate(
            command_queue, channels, baselines, allocator=allocator, **noise_est_args
        )
        self.threshold = template.threshold.instantiate(
            command_queue, channels, baselines, allocator=allocator, **threshold_args
        )
        stages: List[Tuple[str, accel.Operation]] = [("background", self.background)]
        if template.transpose_deviations is not None:
            self.transpose_deviations = template.transpose_deviations.instantiate(
                command_queue, (channels, baselines)
            )
            stages.append(("transpose_deviations", self.transpose_deviations))
        stages.append(("noise_est", self.noise_est))
        stages.append(("threshold", self.threshold))
        if template.transpose_flags is not None:
            self.transpose_flags = template.transpose_flags.instantiate(
                command_queue, (baselines, channels)
            )
            stages.append(("transpose_flags", self.transpose_flags))

        # which layout each consumer reads decides which compound it joins
        dev_of_noise = "deviations_t" if self.noise_est.transposed else "deviations"
        dev_of_threshold = "deviations_t" if self.threshold.transposed else "deviations"
        flags_of_threshold = "flags_t" if self.threshold.transposed else "flags"
        compounds = {
            "vis": ["background:vis"],
            "input_flags": ["background:flags"],
            "deviations": ["background:deviations", "transpose_deviations:src"],
            "deviations_t": ["transpose_deviations:dest"],
            "noise": ["noise_est:noise", "threshold:noise"],
            "flags_t": ["transpose_flags:src"],
            "flags": ["transpose_flags:dest"],
        }
        compounds[dev_of_noise].append("noise_est:deviations")
        compounds[dev_of_threshold].append("threshold:deviations")
        compounds[flags_of_threshold].append("threshold:flags")
        super().__init__(command_queue, stages, compounds, allocator=allocator)


class FusedFlaggerDevice(accel.Operation):
    """Single-pass flagger: one HIP kernel from visibilities to flags.

    Presents the slots of :class:`FlaggerDevice` that survive fusion. Results are
    bit-identical to ``host.FlaggerHost(BackgroundMedianFilterHost, NoiseEstMADHost,
    ThresholdSumHost | ThresholdSimpleHost)`` because everything after the float32
    amplitude is computed in float64, as the host classes do.

    .. rubric:: Slots

    **vis** : channels x baselines, complex64 (float32 if the backgrounder takes amplitudes)
    **input_flags** : channels or channels x baselines, uint8 (only with ``use_flags``)
    **noise** : baselines, float32 (float64 estimate rounded once)
    **flags** : channels x baselines, uint8
    .. rubric:: Optional slots (the reference's temporaries, rfi/device.py:1081-1150)

    **deviations** : channels x baselines, float32
    **deviations_t** : baselines x channels, float32
    **flags_t** : baselines x channels, uint8

    The fused kernel needs none of them, so :meth:`ensure_all_bound` leaves them alone
    (``deviations`` excepted if the template was built with ``keep_deviations=True``). They
    exist all the same: binding one, or asking for it with :meth:`buffer` (which allocates
    it), makes every later call fill it -- ``deviations`` by the kernel itself (13 instead of
    9 bytes per sample, and the 4-baseline kernel instead of the persistent one), the
    transposed ones by a transpose behind it. A buffer materialised after a call holds
    nothing until the next call.
    """

    _OPTIONAL = ("deviations", "deviations_t", "flags_t")

    def __init__(self, template: FlaggerDeviceTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, threshold_args: Mapping[str, Any] = {},
                 allocator: Optional[AbstractAllocator] = None, vis_pad: int = 0) -> None:  # fmt: skip
        super().__init__(command_queue, allocator)
        if vis_pad < 0 or vis_pad % 2:
            raise ValueError("vis_pad must be even and not negative")
        self.template = template
        self.kernel = template._fused_kernel
        self.channels = channels
        self.baselines = baselines
        bg = template.background
        th = template.threshold
        args = dict(threshold_args)
        if "n_sigma" not in args:
            raise TypeError("threshold_args must provide n_sigma")
        self.n_sigma = float(args.pop("n_sigma"))
        if isinstance(th, ThresholdSumDeviceTemplate):
            falloff = float(args.pop("threshold_falloff", _THRESHOLD_SUM_DEFAULT_THRESHOLD_FALLOFF))
            self.threshold_kind = 1
            self.n_windows = th.n_windows
            self.scales = ctypes_double_array([pow(falloff, -i) for i in range(th.n_windows)])
        else:
            self.threshold_kind = 0
            self.n_windows = 1
            self.scales = ctypes_double_array([1.0])
        if args:
            raise TypeError(f"unexpected threshold arguments {sorted(args)}")
        vis_type = np.float32 if bg.is_amplitude else np.complex64
        # 16-byte loads of baseline pairs want an even row stride; `vis_pad` more elements
        # per row where that stride suits the memory system better (template's `tuning`)
        self.vis_pad = vis_pad
        self.slots["vis"] = accel.IOSlot(
            (channels, accel.Dimension(baselines, min_padded_size=baselines + vis_pad, alignment=2)),
            vis_type,
        )
        if bg.use_flags == BackgroundFlags.FULL:
            self.slots["input_flags"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.uint8)
        elif bg.use_flags == BackgroundFlags.CHANNEL:
            self.slots["input_flags"] = accel.IOSlot((channels,), np.uint8)
        self.slots["noise"] = accel.IOSlot((baselines,), np.float32)
        # flags and deviations are shared with the source slots of two transposes that only
        # run when somebody has bound their destinations (the reference's flags_t / deviations_t)
        context = command_queue.context
        self._transpose_dev = transpose.TransposeTemplate(context, np.float32, "float").instantiate(
            command_queue, (channels, baselines), allocator=allocator)
        self._transpose_flags = transpose.TransposeTemplate(
            context, np.uint8, "unsigned char").instantiate(
            command_queue, (channels, baselines), allocator=allocator)
        self.slots["flags"] = accel.CompoundIOSlot([
            accel.IOSlot((channels, accel.Dimension(baselines)), np.uint8),
            self._transpose_flags.slots["src"]])
        self.slots["deviations"] = accel.CompoundIOSlot([
            accel.IOSlot((channels, accel.Dimension(baselines)), np.float32),
            self._transpose_dev.slots["src"]])
        self.slots["deviations_t"] = self._transpose_dev.slots["dest"]
        self.slots["flags_t"] = self._transpose_flags.slots["dest"]
        self._mandatory = [name for name in self.slots
                           if name not in self._OPTIONAL
                           or (name == "deviations" and template.keep_deviations)]
        # scheduling counters of the kernel (64 bytes, zeroed once; not a slot: nothing a
        # caller could usefully bind)
        self._workspace = accel.DeviceArray(command_queue.context, (16,), np.uint32)
        self._workspace.zero(command_queue)
        self._armed = None

    def ensure_all_bound(self) -> None:
        for name in self._mandatory:
            self.ensure_bound(name)

    def buffer(self, name: str) -> accel.DeviceArray:
        if name in self._OPTIONAL and not self.slots[name].is_bound():
            self.ensure_bound(name)  # materialise: filled by every call from now on
        return super().buffer(name)

    def required_bytes(self) -> int:
        return sum(slot.required_bytes() for name, slot in self.slots.items()
                   if name in self._mandatory or slot.is_bound())

    def _run(self) -> None:
        bg = self.template.background
        vis = self.buffer("vis")
        flags = self.buffer("flags")
        in_flags = self.buffer("input_flags") if bg.use_flags else None
        want_dev_t = self.slots["deviations_t"].is_bound()
        if want_dev_t:
            self.ensure_bound("deviations")
        dev = super().buffer("deviations") if self.slots["deviations"].is_bound() else None
        in_flags_stride = in_flags.padded_shape[1] if bg.use_flags == BackgroundFlags.FULL else 0
        self.command_queue.enqueue_kernel(
            self.kernel,
            [
                vis.buffer,
                in_flags.buffer if in_flags is not None else None,
                flags.buffer,
                dev.buffer if dev is not None else None,
                self.buffer("noise").buffer,
                np.int32(self.channels),
                np.int32(self.baselines),
                np.int32(vis.padded_shape[1]),
                np.int32(in_flags_stride),
                np.int32(flags.padded_shape[1]),
                np.int32(dev.padded_shape[1] if dev is not None else 0),
                np.int32(bg.width),
                np.int32(bg.is_amplitude),
                np.int32(bg.use_flags.value),
                np.int32(self.threshold_kind),
                float(self.n_sigma),
                self.scales,
                np.int32(self.n_windows),
                np.int32(self.template.threshold.flag_value),
                self._workspace.buffer,
            ],
        )
        self._armed = None  # (events of profile_next_run are recorded now: ours to drop)
        if want_dev_t:
            self._transpose_dev()
        if self.slots["flags_t"].is_bound():
            self._transpose_flags()

    def profile_next_run(self):
        """Arm two events around the flagger kernel of the next call (excluding the
        zero-fill of `flags` that precedes it); returns (start, stop). After the queue
        has finished, ``stop.time_since(start)`` is that kernel's duration."""
        queue = self.command_queue
        start, stop = queue.create_event(), queue.create_event()
        _lib.call("ksp_flagger_fused_profile", ctypes.c_void_p(start.handle),
                  ctypes.c_void_p(stop.handle))  # fmt: skip
        self._armed = (start, stop)  # alive until the call, whatever the caller does with them
        return start, stop

    def parameters(self) -> Mapping[str, Any]:
        return {
            "fused": True,
            "vis_pad": self.vis_pad,
            "keep_deviations": self.slots["deviations"].is_bound(),
            "width": self.template.background.width,
            "n_sigma": self.n_sigma,
            "n_windows": self.n_windows,
            "channels": self.channels,
            "baselines": self.baselines,
        }


class FlaggerHostFromDevice(host.AbstractFlaggerHost):
    """Make a :class:`FlaggerDeviceTemplate` callable like ``host.FlaggerHost``
    (reference rfi/device.py:1169-1222); allocates on every call."""

    def __init__(self, template: FlaggerDeviceTemplate, command_queue: AbstractCommandQueue,
                 background_args: Mapping[str, Any] = {}, noise_est_args: Mapping[str, Any] = {},
                 threshold_args: Mapping[str, Any] = {}) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue
        self.background_args = dict(background_args)
        self.noise_est_args = dict(noise_est_args)
        self.threshold_args = dict(threshold_args)

    def __call__(self, vis: np.ndarray, input_flags: Optional[np.ndarray] = None) -> np.ndarray:
        _native_op.check_optional(input_flags, self.template.background.use_flags, "channel flags")
        channels, baselines = vis.shape
        fn = self.template.instantiate(
            self.command_queue, channels, baselines, self.background_args, self.noise_est_args,
            self.threshold_args,
        )  # fmt: skip
        inputs = {"vis": vis, "input_flags": input_flags}
        return _native_op.run_once(fn, self.command_queue, inputs, ["flags"])[0]


# ------------------------------------------------------------------------ flag counts
class FlagCountTemplate(_native_op.NativeTemplate):
    """Count flagged samples per channel and per baseline, on the device (no reference
    counterpart: the reference's callers count on a host copy of the flags).

    One kernel reads every flag byte once and produces both sets of counts, for up to 8
    masks at a time; see :class:`host.FlagCountHost` for what is counted.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    masks
        1 to 8 integers in 1..255: a sample counts for a mask when its flag byte has any
        of the mask's bits set. Default ``(0xFF,)``: any flag. ``ValueError`` for an empty or
        too long sequence or a value out of range, ``TypeError`` for a non-integer.
    transposed
        ``False`` (default): `flags` is channels x baselines, the flagger's output.
        ``True``: baselines x channels. The counts are the same either way.
    accumulate
        ``False`` (default): every call overwrites both outputs. ``True``: a call adds to
        what the outputs hold (zero them first); the sums wrap modulo 2**32.
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.FlagCountHost
    KERNEL = "ksp_flag_count"

    def __init__(self, context: AbstractContext, masks=(0xFF,), transposed: bool = False,
                 accumulate: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.masks = host.check_flag_masks(masks)
        self.transposed = bool(transposed)
        self.accumulate = bool(accumulate)
        self._setup(context, tuning)


class FlagCount(_native_op.NativeOperation):
    """Concrete :class:`FlagCountTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1).

    .. rubric:: Slots

    **flags** : channels x baselines (baselines x channels if transposed), uint8
    **channel_counts** : len(masks) x channels, uint32
    **baseline_counts** : len(masks) x baselines, uint32
    """

    def __init__(self, template: FlagCountTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        _check_shape(channels, baselines)
        self.transposed = template.transposed
        self.masks = (ctypes.c_uint8 * len(template.masks))(*template.masks)
        shape = self.layout(self.transposed)
        n_masks = len(template.masks)
        self.slots["flags"] = accel.IOSlot((shape[0], accel.Dimension(shape[1])), np.uint8)
        self.slots["channel_counts"] = accel.IOSlot(
            (n_masks, accel.Dimension(channels)), np.uint32)  # fmt: skip
        self.slots["baseline_counts"] = accel.IOSlot(
            (n_masks, accel.Dimension(baselines)), np.uint32)  # fmt: skip

    def _run(self) -> None:
        flags = self.buffer("flags")
        # the kernel counts over rows and columns of `flags` as it lies in memory
        names = ("baseline_counts", "channel_counts") if self.transposed else (
            "channel_counts", "baseline_counts")  # fmt: skip
        row_counts, col_counts = self.buffer(names[0]), self.buffer(names[1])
        self._launch(
            flags.buffer,
            row_counts.buffer,
            col_counts.buffer,
            np.int32(flags.shape[0]),
            np.int32(flags.shape[1]),
            np.int32(flags.padded_shape[1]),
            np.int32(row_counts.padded_shape[1]),
            np.int32(col_counts.padded_shape[1]),
            self.masks,
            np.int32(len(self.masks)),
            np.int32(self.template.accumulate),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            masks=self.template.masks,
            transposed=self.transposed,
            accumulate=self.template.accumulate,
        )


FlagCountTemplate.operation_class = FlagCount


class FlagCountHostFromDevice:
    """Make a :class:`FlagCountTemplate` callable like :class:`host.FlagCountHost`:
    channel-major `flags` in, ``(channel_counts, baseline_counts)`` out; allocates on every
    call. ``ValueError`` for a template that accumulates (a call has nothing to add to)."""

    def __init__(self, template: FlagCountTemplate, command_queue: AbstractCommandQueue) -> None:
        if template.accumulate:
            raise ValueError("the template accumulates: there is no single call's result")
        self.template = template
        self.command_queue = command_queue

    def __call__(self, flags: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        channels, baselines = flags.shape
        fn = self.template.instantiate(self.command_queue, channels, baselines)
        if self.template.transposed:
            flags = flags.T
        return tuple(_native_op.run_once(fn, self.command_queue, {"flags": flags},
                                         ["channel_counts", "baseline_counts"]))  # fmt: skip


# ------------------------------------------------------------ scale-invariant rank
SIR_MAX_CHANNELS = 262144


class ScaleInvariantRankTemplate(_native_op.NativeTemplate):
    """Scale-invariant rank (SIR) extension of flags along the channel axis, in place, on the
    device (no reference counterpart); see :class:`host.ScaleInvariantRankHost` for the rule,
    which the kernels match bit for bit.

    It belongs between a flagger and whatever consumes its flags (:class:`FlagCount`,
    :class:`Accumulate`): all of them have a ``flags`` slot of the same shape, to be shared
    through the ``compounds`` of an :class:`.accel.OperationSequence`.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    eta, mask, flag_value
        As for :class:`host.ScaleInvariantRankHost` (same errors). ``eta_q`` is the quantised
        `eta` the kernel gets.
    transposed
        ``False`` (default): `flags` is channels x baselines, the flagger's output.
        ``True``: baselines x channels, the layout of ``ThresholdSum(transposed=True)``.
        Channels are the axis of the operator either way.
    tuning
        The kernels pick their launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.ScaleInvariantRankHost
    KERNEL = "ksp_sir"

    def __init__(self, context: AbstractContext, eta: float, mask: int = 0xFF,
                 flag_value: int = 1, transposed: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        checked = host.ScaleInvariantRankHost(eta, mask, flag_value)
        self.eta = checked.eta
        self.eta_q = checked.eta_q
        self.mask = checked.mask
        self.flag_value = checked.flag_value
        self.transposed = bool(transposed)
        self._setup(context, tuning)


class ScaleInvariantRank(_native_op.NativeOperation):
    """Concrete :class:`ScaleInvariantRankTemplate` (``ValueError`` if `channels` or
    `baselines` is below 1, or `channels` above 262144).

    .. rubric:: Slots

    **flags** : channels x baselines (baselines x channels if transposed), uint8, in and out
    """

    MAX_CHANNELS_SUPPORTED = SIR_MAX_CHANNELS

    def __init__(self, template: ScaleInvariantRankTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        _check_shape(channels, baselines)
        if channels > self.MAX_CHANNELS_SUPPORTED:
            raise ValueError(f"at most {self.MAX_CHANNELS_SUPPORTED} channels")
        self.transposed = template.transposed
        shape = self.layout(self.transposed)
        self.slots["flags"] = accel.IOSlot((shape[0], accel.Dimension(shape[1])), np.uint8)

    def _run(self) -> None:
        flags = self.buffer("flags")
        self._launch(
            flags.buffer,
            np.int32(flags.shape[0]),
            np.int32(flags.shape[1]),
            np.int32(flags.padded_shape[1]),
            np.int32(1 if self.transposed else 0),  # the axis the lines run along
            np.int32(self.template.eta_q),
            np.int32(self.template.mask),
            np.int32(self.template.flag_value),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            eta_q=self.template.eta_q,
            mask=self.template.mask,
            flag_value=self.template.flag_value,
            transposed=self.transposed,
        )


ScaleInvariantRankTemplate.operation_class = ScaleInvariantRank


class ScaleInvariantRankHostFromDevice:
    """Make a :class:`ScaleInvariantRankTemplate` callable like
    :class:`host.ScaleInvariantRankHost`: channel-major `flags` in, a new array out;
    allocates on every call."""

    def __init__(self, template: ScaleInvariantRankTemplate,
                 command_queue: AbstractCommandQueue) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue

    def __call__(self, flags: np.ndarray) -> np.ndarray:
        channels, baselines = flags.shape
        fn = self.template.instantiate(self.command_queue, channels, baselines)
        if self.template.transposed:
            flags = flags.T
        out = _native_op.run_once(fn, self.command_queue, {"flags": flags}, ["flags"])[0]
        return np.ascontiguousarray(out.T) if self.template.transposed else out


# -------------------------------------------------------------------------- averaging
def _check_average_shape(channels: int, channel_factor: int) -> None:
    if channel_factor < 1 or channels % channel_factor:
        raise ValueError("channel_factor must be at least 1 and divide channels")


class AccumulateTemplate(_native_op.NativeTemplate):
    """Add one dump of visibilities to device-resident accumulators, leaving flagged
    samples out (no reference counterpart: the reference's callers average in their own
    code). :class:`host.AveragerHost` defines the arithmetic of ``add``; the kernel matches
    it bit for bit. :class:`FinaliseTemplate` turns the accumulators into averages.

    The accumulators are read, updated and written back by every call: zero them once
    before the first dump (``buffer("acc_vis").zero(queue)`` and likewise for
    ``acc_weights`` and ``acc_flags``); :class:`Finalise` zeroes them again if built with
    ``clear=True``.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    use_weights
        ``True`` (default): there is a `weights` slot. ``False``: every weight is 1.
    input_flags
        :class:`BackgroundFlags`: whether there is an `input_flags` slot that is ORed into
        the flags, one byte per channel (CHANNEL) or per sample (FULL)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.AveragerHost
    KERNEL = "ksp_average_accumulate"

    def __init__(self, context: AbstractContext, use_weights: bool = True,
                 input_flags: BackgroundFlags = BackgroundFlags.NONE,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.use_weights = bool(use_weights)
        self.input_flags = BackgroundFlags(input_flags)
        self._setup(context, tuning)


class Accumulate(_native_op.NativeOperation):
    """Concrete :class:`AccumulateTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1).

    .. rubric:: Slots

    **vis** : channels x baselines, complex64
    **flags** : channels x baselines, uint8 (any non-zero byte means flagged)
    **weights** : channels x baselines, float32 (only with ``use_weights``)
    **input_flags** : channels or channels x baselines, uint8 (only if the mode is not NONE)
    **acc_vis** : channels x baselines, complex64
    **acc_weights** : channels x baselines, float32
    **acc_flags** : channels x baselines, uint8

    Every two-dimensional slot has a dimension object of its own for the baselines, so
    `vis` and `flags` can be compounded with the flagger's slots of those names and take
    their padding.
    """

    def __init__(self, template: AccumulateTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        _check_shape(channels, baselines)

        def full(dtype) -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        self.slots["vis"] = full(np.complex64)
        self.slots["flags"] = full(np.uint8)
        if template.use_weights:
            self.slots["weights"] = full(np.float32)
        if template.input_flags == BackgroundFlags.FULL:
            self.slots["input_flags"] = full(np.uint8)
        elif template.input_flags == BackgroundFlags.CHANNEL:
            self.slots["input_flags"] = accel.IOSlot((channels,), np.uint8)
        self.slots["acc_vis"] = full(np.complex64)
        self.slots["acc_weights"] = full(np.float32)
        self.slots["acc_flags"] = full(np.uint8)

    def _run(self) -> None:
        mode = self.template.input_flags
        vis, flags = self.buffer("vis"), self.buffer("flags")
        weights = self.buffer("weights") if self.template.use_weights else None
        in_flags = self.buffer("input_flags") if mode else None
        acc = [self.buffer(name) for name in ("acc_vis", "acc_weights", "acc_flags")]
        self._launch(
            vis.buffer,
            flags.buffer,
            _native_op.pointer(weights),
            _native_op.pointer(in_flags),
            np.int32(mode.value),
            acc[0].buffer,
            acc[1].buffer,
            acc[2].buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(vis.padded_shape[1]),
            np.int32(flags.padded_shape[1]),
            _native_op.stride(weights),
            np.int32(in_flags.padded_shape[1] if mode == BackgroundFlags.FULL else 0),
            np.int32(acc[0].padded_shape[1]),
            np.int32(acc[1].padded_shape[1]),
            np.int32(acc[2].padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            use_weights=self.template.use_weights, input_flags=self.template.input_flags.name
        )


AccumulateTemplate.operation_class = Accumulate


class FinaliseTemplate(_native_op.NativeTemplate):
    """Turn the accumulators of :class:`Accumulate` into averages: sum every
    `channel_factor` adjacent channels in order, divide by the summed weight, and report the
    flags of outputs whose contributions were all flagged (:meth:`host.AveragerHost.finalise`,
    matched bit for bit).

    Parameters
    ----------
    context
        Context whose device will run the kernel
    channel_factor
        Number of adjacent channels per output channel, at least 1 (``ValueError``); it
        must divide the channels given to :meth:`instantiate` (``ValueError`` there)
    clear
        ``True`` (default): the kernel zeroes the accumulators it has read, in the same
        pass, ready for the next dump. ``False``: they are left as they are.
    tuning
        Nothing to tune, any key is a ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.AveragerHost
    KERNEL = "ksp_average_finalise"

    def __init__(self, context: AbstractContext, channel_factor: int = 1, clear: bool = True,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        if channel_factor < 1:
            raise ValueError("channel_factor must be at least 1")
        self.channel_factor = int(channel_factor)
        self.clear = bool(clear)
        self._setup(context, tuning)


class Finalise(_native_op.NativeOperation):
    """Concrete :class:`FinaliseTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1 or the template's `channel_factor` does not divide `channels`).

    .. rubric:: Slots

    **acc_vis** : channels x baselines, complex64
    **acc_weights** : channels x baselines, float32
    **acc_flags** : channels x baselines, uint8
    **vis** : channels // channel_factor x baselines, complex64
    **weights** : channels // channel_factor x baselines, float32
    **flags** : channels // channel_factor x baselines, uint8
    """

    def __init__(self, template: FinaliseTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        _check_shape(channels, baselines)
        _check_average_shape(channels, template.channel_factor)
        out_channels = channels // template.channel_factor
        for prefix, rows in (("acc_", channels), ("", out_channels)):
            for name, dtype in (("vis", np.complex64), ("weights", np.float32), ("flags", np.uint8)):
                self.slots[prefix + name] = accel.IOSlot(
                    (rows, accel.Dimension(baselines)), dtype)  # fmt: skip

    def _run(self) -> None:
        names = ("acc_vis", "acc_weights", "acc_flags", "vis", "weights", "flags")
        buffers = [self.buffer(name) for name in names]
        self._launch(
            *[b.buffer for b in buffers],
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.template.channel_factor),
            np.int32(self.template.clear),
            *[np.int32(b.padded_shape[1]) for b in buffers],
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters(
            channel_factor=self.template.channel_factor, clear=self.template.clear
        )


FinaliseTemplate.operation_class = Finalise


class AveragerHostFromDevice:
    """Present an :class:`AccumulateTemplate` and a :class:`FinaliseTemplate` through the
    ``add`` / ``finalise`` interface of :class:`host.AveragerHost`. The operations are
    instantiated and the shared accumulators allocated and zeroed once, here; with a
    `finalise_template` built with ``clear=False`` the accumulators keep their sums across
    :meth:`finalise`, unlike the host class."""

    def __init__(self, accumulate_template: AccumulateTemplate,
                 finalise_template: FinaliseTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int) -> None:  # fmt: skip
        self.command_queue = command_queue
        self.input_flags = accumulate_template.input_flags
        self.use_weights = accumulate_template.use_weights
        self._accumulate = accumulate_template.instantiate(command_queue, channels, baselines)
        self._finalise = finalise_template.instantiate(command_queue, channels, baselines)
        shared = ("acc_vis", "acc_weights", "acc_flags")
        self._sequence = accel.OperationSequence(
            command_queue, [("accumulate", self._accumulate), ("finalise", self._finalise)],
            compounds={name: ["accumulate:" + name, "finalise:" + name] for name in shared})
        self._sequence.ensure_all_bound()
        for name in shared:
            self._sequence.buffer(name).zero(command_queue)

    def add(self, vis: np.ndarray, flags: np.ndarray, weights: Optional[np.ndarray] = None,
            input_flags: Optional[np.ndarray] = None) -> None:  # fmt: skip
        _native_op.check_optional(input_flags, self.input_flags, "input_flags")
        if weights is not None and not self.use_weights:
            raise TypeError("weights were provided but not included in the template")
        fn = self._accumulate
        if self.use_weights and weights is None:
            weights = np.ones(fn.buffer("weights").shape, np.float32)
        inputs = {"vis": vis, "flags": flags, "weights": weights, "input_flags": input_flags}
        _native_op.run_once(fn, self.command_queue, inputs, [])

    def finalise(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return tuple(_native_op.run_once(self._finalise, self.command_queue, {},
                                         ["vis", "weights", "flags"]))  # fmt: skip
