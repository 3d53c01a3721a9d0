"""The step in front of the flagging chain: a correlator's integer dump, as it arrives, to the
``vis``, ``input_flags`` and ``weights`` that :mod:`.device` takes as inputs, in one kernel
launch (no reference counterpart). :class:`.host.PrepareHost` is the definition; the kernel
matches it bit for bit, static channel masks chosen per baseline and flags per baseline
included. And the step behind it: the float32 ``weights`` that
:class:`.device.Finalise` leaves to one byte per sample and one float32 per channel, again in
one launch and bit for bit what :class:`.host.CompressWeightsHost` defines. And the step that
closes it: the percentiles of the averaged amplitudes over ranges of baselines, flagged and NaN
samples left out, with a count and the OR of the flags per range and channel: all ranges in one
launch, bit for bit what :class:`.host.RangePercentilesHost` defines. And its companion: per
baseline and for up to eight series of channel weights, the weighted means of the visibility and
of its amplitude over the channels that carry data, with the weight sum, a count and the OR of
the flags, every sample read once, bit for bit what :class:`.host.BandAverageHost` defines. And
the step in its middle, for a pipeline that holds several dumps: a block of up to eight dumps
added to the accumulators of :class:`.device.Accumulate` in one launch that reads and writes
them once, bit for bit what as many calls of :meth:`.host.AveragerHost.add` leave. And the step
between averaging and the consumers of calibrated data: per-input gain corrections applied to
``vis``, ``weights`` and ``flags`` in one launch, in place or not, bit for bit what
:class:`.host.ApplyGainsHost` defines. And what produces those gains: per channel, the
per-input gains of a point source solved with StEFCal in one launch, one workgroup per channel,
bit for bit what :class:`.host.SolveGainsHost` defines (for arrays of up to 512 inputs, with the
matrices in a work area: :class:`.host.SolveGainsLargeHost`). And the step in front of that for a
field
that is not one source at the phase centre: the model visibilities of up to 64 point sources,
with float64 phases, and optionally the data divided by them, in one launch, bit for bit what
:class:`.host.PredictHost` defines. And the step behind the solver: per input, the delay and
phase fitted to the solved gains across the band and the smooth phasor that is applied in their
place, in one launch with one workgroup per input, bit for bit what
:class:`.host.FitDelaysHost` defines. And the step that makes a table for a target scan of
both: per input, the solved gains with the delay divided out, smoothed, normalised, filled
across the channels the solver lost, and recombined with the delay and a band-wide gain, in one
launch with one workgroup per input, bit for bit what :class:`.host.InterpolateGainsHost`
defines. And the step that closes the dual-polarisation chain: the per-antenna 2x2 Jones
matrices of the leakage solve applied to the four products of every antenna pair, with the
weights propagated and the flags ORed over the pair, in one launch, in place or not, bit for bit
what :class:`.host.ApplyJonesHost` defines. And what joins the two halves of that chain: the
solved matrices filled whole across the channels the solver lost, per antenna, with a delay
model per feed, in one launch, bit for bit what :class:`.host.InterpolateJonesHost` defines,
and the diagonal of the matrices as the gains a delay fit reads
(:class:`.host.JonesDiagonalHost`). The classes follow DESIGN.md, "Adding an operation".
"""

import ctypes
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from .. import _native_op, accel
from ..abc import AbstractCommandQueue, AbstractContext
from ..accel import AbstractAllocator
from . import host


class PrepareTemplate(_native_op.NativeTemplate):
    """Gather the baselines the pipeline keeps from a dump of saturating int32 (re, im)
    accumulations, scale them to complex64, mark the samples the correlator never received
    and, optionally, derive weights from the autocorrelations; see :class:`host.PrepareHost`
    for every step.

    The three outputs are the inputs of the rest of the chain: ``vis`` and ``input_flags`` are
    the slots of those names of the fused flagger (``use_flags=BackgroundFlags.FULL``) and of
    :class:`.device.Accumulate` (``input_flags=BackgroundFlags.FULL``), ``weights`` is
    :class:`.device.Accumulate`'s; share them through the ``compounds`` of an
    :class:`.accel.OperationSequence`.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    scale, lost_flag, weight_scale
        As for :class:`host.PrepareHost` (same errors)
    channel_flags
        ``True``: there is a `channel_flags` slot, one byte per channel that is ORed into
        every sample of its channel
    weights
        ``True``: there are an `auto_source` and a `weights` slot
    mask_classes
        0 .. 8 (``ValueError``). 1 or more: the `channel_flags` slot holds that many static
        masks, one per row, and there is a `mask_index` slot that names the row of every
        baseline (a value of `mask_classes` or more: none). Needs `channel_flags`
        (``ValueError``).
    baseline_flags
        ``True``: there is a `baseline_flags` slot, one byte per baseline that is ORed into
        every sample of its baseline
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.PrepareHost
    KERNEL = "ksp_prepare"
    #: the launcher of a template with `mask_classes` or `baseline_flags`
    FLAGS_KERNEL = "ksp_prepare_flags"

    def __init__(self, context: AbstractContext, scale: float = 1.0, lost_flag: int = 8,
                 channel_flags: bool = False, weights: bool = False, weight_scale: float = 1.0,
                 mask_classes: int = 0, baseline_flags: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        checked = host.PrepareHost(scale, lost_flag, weight_scale)
        self.scale = checked.scale
        self.lost_flag = checked.lost_flag
        self.weight_scale = checked.weight_scale
        self.channel_flags = bool(channel_flags)
        self.weights = bool(weights)
        self.mask_classes = int(mask_classes)
        self.baseline_flags = bool(baseline_flags)
        if not 0 <= self.mask_classes <= host.PrepareHost.MAX_CLASSES:
            raise ValueError(f"mask_classes must be 0..{host.PrepareHost.MAX_CLASSES}")
        if self.mask_classes >= 1 and not self.channel_flags:
            raise ValueError("mask_classes of 1 or more need channel_flags")
        self._setup(context, tuning)
        self.per_baseline = self.mask_classes >= 1 or self.baseline_flags
        if self.per_baseline:
            self.kernel = context.native_kernel(self.FLAGS_KERNEL)


class Prepare(_native_op.NativeOperation):
    """Concrete :class:`PrepareTemplate` (``ValueError`` if `channels`, `baselines` or
    `in_baselines` is below 1). `in_baselines`, the number of baselines of the dump, defaults
    to `baselines`, the number the pipeline keeps.

    .. rubric:: Slots

    **vis_in** : channels x in_baselines x 2, int32, (re, im)
    **source** : baselines, int32: the input baseline of every output baseline
    **channel_flags** : channels, uint8 (only with ``channel_flags``); with ``mask_classes``
    of 1 or more: mask_classes x channels
    **mask_index** : baselines, uint8 (only with ``mask_classes`` of 1 or more)
    **baseline_flags** : baselines, uint8 (only with ``baseline_flags``)
    **auto_source** : baselines x 2, int32: the input baselines of the two autocorrelations
    of every output baseline (only with ``weights``)
    **vis** : channels x baselines, complex64
    **input_flags** : channels x baselines, uint8
    **weights** : channels x baselines, float32 (only with ``weights``)

    Every padded dimension is an object of its own, so each output can be compounded with
    its consumer's slot and take its padding.
    """

    def __init__(self, template: PrepareTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, in_baselines: Optional[int] = None,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if in_baselines is None:
            in_baselines = baselines
        if channels < 1 or baselines < 1 or in_baselines < 1:
            raise ValueError("channels, baselines and in_baselines must be at least 1")
        self.in_baselines = in_baselines

        def pair() -> accel.Dimension:
            return accel.Dimension(2, exact=True)

        def full(dtype) -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        self.slots["vis_in"] = accel.IOSlot(
            (channels, accel.Dimension(in_baselines), pair()), np.int32)  # fmt: skip
        self.slots["source"] = accel.IOSlot((accel.Dimension(baselines),), np.int32)
        if template.mask_classes >= 1:
            self.slots["channel_flags"] = accel.IOSlot(
                (accel.Dimension(template.mask_classes, exact=True), accel.Dimension(channels)),
                np.uint8)  # fmt: skip
            self.slots["mask_index"] = accel.IOSlot((accel.Dimension(baselines),), np.uint8)
        elif template.channel_flags:
            self.slots["channel_flags"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)
        if template.baseline_flags:
            self.slots["baseline_flags"] = accel.IOSlot((accel.Dimension(baselines),), np.uint8)
        if template.weights:
            self.slots["auto_source"] = accel.IOSlot(
                (accel.Dimension(baselines), pair()), np.int32)  # fmt: skip
        self.slots["vis"] = full(np.complex64)
        self.slots["input_flags"] = full(np.uint8)
        if template.weights:
            self.slots["weights"] = full(np.float32)

    def _run(self) -> None:
        template = self.template
        vis_in, source = self.buffer("vis_in"), self.buffer("source")
        channel_flags = self.buffer("channel_flags") if template.channel_flags else None
        auto_source = self.buffer("auto_source") if template.weights else None
        vis, input_flags = self.buffer("vis"), self.buffer("input_flags")
        weights = self.buffer("weights") if template.weights else None
        if template.per_baseline:
            self._run_flags(vis_in, source, channel_flags, auto_source, vis, input_flags, weights)
            return
        self._launch(
            vis_in.buffer,
            source.buffer,
            _native_op.pointer(auto_source),
            _native_op.pointer(channel_flags),
            vis.buffer,
            input_flags.buffer,
            _native_op.pointer(weights),
            np.int32(self.channels),
            np.int32(self.in_baselines),
            np.int32(self.baselines),
            np.int32(vis_in.padded_shape[1]),
            np.int32(vis.padded_shape[1]),
            np.int32(input_flags.padded_shape[1]),
            _native_op.stride(weights),
            np.float32(template.scale),
            np.float32(template.weight_scale),
            np.int32(template.lost_flag),
        )

    def _run_flags(self, vis_in, source, channel_flags, auto_source, vis, input_flags,
                   weights) -> None:  # fmt: skip
        """Launch ``ksp_prepare_flags``: the arguments of ``ksp_prepare`` and `mask_index`,
        `baseline_flags`, the number of classes and the row stride of `channel_flags`."""
        template = self.template
        classes = template.mask_classes
        mask_index = self.buffer("mask_index") if classes >= 1 else None
        baseline_flags = self.buffer("baseline_flags") if template.baseline_flags else None
        self._launch(
            vis_in.buffer,
            source.buffer,
            _native_op.pointer(auto_source),
            _native_op.pointer(channel_flags),
            _native_op.pointer(mask_index),
            _native_op.pointer(baseline_flags),
            vis.buffer,
            input_flags.buffer,
            _native_op.pointer(weights),
            np.int32(self.channels),
            np.int32(self.in_baselines),
            np.int32(self.baselines),
            np.int32(classes),
            np.int32(vis_in.padded_shape[1]),
            np.int32(channel_flags.padded_shape[1] if classes >= 1 else 0),
            np.int32(vis.padded_shape[1]),
            np.int32(input_flags.padded_shape[1]),
            _native_op.stride(weights),
            np.float32(template.scale),
            np.float32(template.weight_scale),
            np.int32(template.lost_flag),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        own = dict(
            scale=float(template.scale),
            lost_flag=template.lost_flag,
            channel_flags=template.channel_flags,
            weights=template.weights,
            weight_scale=float(template.weight_scale),
            in_baselines=self.in_baselines,
        )
        # (only when they are on: without them this is the dict it always was)
        if template.mask_classes >= 1:
            own["mask_classes"] = template.mask_classes
        if template.baseline_flags:
            own["baseline_flags"] = True
        return self._parameters(**own)


PrepareTemplate.operation_class = Prepare


class PrepareHostFromDevice:
    """Make a :class:`PrepareTemplate` callable like :class:`host.PrepareHost`:
    ``(vis_in, source, channel_flags=None, auto_source=None, baseline_flags=None,
    mask_index=None)`` in, ``(vis, input_flags, weights or None)`` out; allocates on every
    call. ``TypeError`` unless each optional input is given exactly when the template has it
    (`mask_index`: with ``mask_classes`` of 1 or more, and `channel_flags` then has that many
    rows, ``ValueError`` otherwise)."""

    def __init__(self, template: PrepareTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis_in: np.ndarray, source: np.ndarray,
                 channel_flags: Optional[np.ndarray] = None,
                 auto_source: Optional[np.ndarray] = None,
                 baseline_flags: Optional[np.ndarray] = None,
                 mask_index: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:  # fmt: skip
        template = self.template
        _native_op.check_optional(channel_flags, template.channel_flags, "channel_flags")
        _native_op.check_optional(auto_source, template.weights, "auto_source")
        _native_op.check_optional(baseline_flags, template.baseline_flags, "baseline_flags")
        _native_op.check_optional(mask_index, template.mask_classes >= 1, "mask_index")
        if mask_index is not None and np.shape(channel_flags)[:-1] != (template.mask_classes,):
            raise ValueError(f"channel_flags must have {template.mask_classes} rows, the "
                             f"template's mask_classes, not shape {np.shape(channel_flags)}")
        channels, in_baselines = vis_in.shape[:2]
        fn = template.instantiate(self.command_queue, channels, source.shape[0], in_baselines)
        inputs = {"vis_in": vis_in, "source": source, "channel_flags": channel_flags,
                  "auto_source": auto_source, "baseline_flags": baseline_flags,
                  "mask_index": mask_index}  # fmt: skip
        outputs = ["vis", "input_flags"] + (["weights"] if template.weights else [])
        out = _native_op.run_once(fn, self.command_queue, inputs, outputs)
        return out[0], out[1], (out[2] if template.weights else None)


class CompressWeightsTemplate(_native_op.NativeTemplate):
    """The step behind the chain: the float32 ``weights`` that :class:`.device.Finalise`
    leaves as one byte per sample (``weights8``) and one float32 per channel
    (``weights_channel``, the row's largest weight divided by 255), in one kernel launch; see
    :class:`host.CompressWeightsHost` for every step. The output of the chain is then 9 bytes
    per sample and 4 per channel instead of 13 per sample.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.CompressWeightsHost
    KERNEL = "ksp_compress_weights"

    def __init__(self, context: AbstractContext,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self._setup(context, tuning)


class CompressWeights(_native_op.NativeOperation):
    """Concrete :class:`CompressWeightsTemplate` (``ValueError`` if `channels` or `baselines`
    is below 1).

    .. rubric:: Slots

    **weights** : channels x baselines, float32
    **weights8** : channels x baselines, uint8
    **weights_channel** : channels, float32

    Every padded dimension is an object of its own, so ``weights`` can be compounded with
    :class:`.device.Finalise`'s ``weights`` and take its padding.
    """

    def __init__(self, template: CompressWeightsTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self.slots["weights"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.float32)
        self.slots["weights8"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.uint8)
        self.slots["weights_channel"] = accel.IOSlot((accel.Dimension(channels),), np.float32)

    def _run(self) -> None:
        weights, weights8 = self.buffer("weights"), self.buffer("weights8")
        self._launch(
            weights.buffer,
            weights8.buffer,
            self.buffer("weights_channel").buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(weights.padded_shape[1]),
            np.int32(weights8.padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        return self._parameters()


CompressWeightsTemplate.operation_class = CompressWeights


class CompressWeightsHostFromDevice:
    """Make a :class:`CompressWeightsTemplate` callable like
    :class:`host.CompressWeightsHost`: ``weights`` in, ``(weights8, weights_channel)`` out;
    allocates on every call."""

    def __init__(self, template: CompressWeightsTemplate,
                 command_queue: AbstractCommandQueue) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue

    def __call__(self, weights: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        channels, baselines = weights.shape
        fn = self.template.instantiate(self.command_queue, channels, baselines)
        out = _native_op.run_once(fn, self.command_queue, {"weights": weights},
                                  ["weights8", "weights_channel"])  # fmt: skip
        return out[0], out[1]


class ApplyGainsTemplate(_native_op.NativeTemplate):
    """The step between averaging and what consumes calibrated data: the per-input gain
    corrections applied to the ``vis`` that :class:`.device.Finalise` leaves, the ``weights``
    scaled to match and the samples without a correction flagged, in one kernel launch; see
    :class:`host.ApplyGainsHost` for every step. The gains are small (channels x inputs) and
    stay on the device; only their application is per sample.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    weights
        ``True``: there are a `weights` and an `out_weights` slot
    flags
        ``True``: there are a `flags` and an `out_flags` slot
    flag_value
        As for :class:`host.ApplyGainsHost` (same errors)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.ApplyGainsHost
    KERNEL = "ksp_apply_gains"

    def __init__(self, context: AbstractContext, weights: bool = True, flags: bool = True,
                 flag_value: int = 128, tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.weights = bool(weights)
        self.flags = bool(flags)
        self.flag_value = host.ApplyGainsHost(flag_value).flag_value
        self._setup(context, tuning)


class ApplyGains(_native_op.NativeOperation):
    """Concrete :class:`ApplyGainsTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1 or `n_inputs` outside 1..4096).

    .. rubric:: Slots

    **vis**, **out_vis** : channels x baselines, complex64
    **weights**, **out_weights** : channels x baselines, float32 (only with ``weights``)
    **flags**, **out_flags** : channels x baselines, uint8 (only with ``flags``)
    **gains** : channels x n_inputs, complex64: the corrections that multiply
    **inputs** : baselines x 2, int32, contiguous: the two inputs of every baseline

    Every padded dimension is an object of its own, so ``vis``, ``weights`` and ``flags`` can
    be compounded with :class:`.device.Finalise`'s (or :class:`Prepare`'s) outputs and the
    ``out_*`` slots with the inputs of :class:`CompressWeights`, :class:`RangePercentiles` or
    the 2-D flagger, each taking the other's padding. Binding one buffer to ``vis`` and
    ``out_vis`` (and likewise to the other two pairs) applies the gains in place; with buffers
    of their own the inputs are left untouched.
    """

    def __init__(self, template: ApplyGainsTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        if not 1 <= n_inputs <= host.ApplyGainsHost.MAX_INPUTS:
            raise ValueError(f"n_inputs must be 1..{host.ApplyGainsHost.MAX_INPUTS}")
        self.n_inputs = n_inputs

        def pair(name: str, dtype) -> None:
            for slot in (name, "out_" + name):
                self.slots[slot] = accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        pair("vis", np.complex64)
        if template.weights:
            pair("weights", np.float32)
        if template.flags:
            pair("flags", np.uint8)
        self.slots["gains"] = accel.IOSlot((channels, accel.Dimension(n_inputs)), np.complex64)
        self.slots["inputs"] = accel.IOSlot(
            (accel.Dimension(baselines), accel.Dimension(2, exact=True)), np.int32)  # fmt: skip

    def _run(self) -> None:
        template = self.template
        vis, out_vis = self.buffer("vis"), self.buffer("out_vis")
        weights = self.buffer("weights") if template.weights else None
        out_weights = self.buffer("out_weights") if template.weights else None
        flags = self.buffer("flags") if template.flags else None
        out_flags = self.buffer("out_flags") if template.flags else None
        gains = self.buffer("gains")
        self._launch(
            vis.buffer,
            _native_op.pointer(weights),
            _native_op.pointer(flags),
            gains.buffer,
            self.buffer("inputs").buffer,
            out_vis.buffer,
            _native_op.pointer(out_weights),
            _native_op.pointer(out_flags),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_inputs),
            np.int32(vis.padded_shape[1]),
            _native_op.stride(weights),
            _native_op.stride(flags),
            np.int32(gains.padded_shape[1]),
            np.int32(out_vis.padded_shape[1]),
            _native_op.stride(out_weights),
            _native_op.stride(out_flags),
            np.int32(template.flag_value),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(weights=template.weights, flags=template.flags,
                                flag_value=template.flag_value, n_inputs=self.n_inputs)  # fmt: skip


ApplyGainsTemplate.operation_class = ApplyGains


class ApplyGainsHostFromDevice:
    """Make an :class:`ApplyGainsTemplate` callable like :class:`host.ApplyGainsHost`:
    ``(vis, gains, inputs, weights=None, flags=None)`` in, ``(out_vis, out_weights or None,
    out_flags or None)`` out; allocates on every call. ``TypeError`` unless `weights` and
    `flags` are each given exactly when the template has them."""

    def __init__(self, template: ApplyGainsTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis: np.ndarray, gains: np.ndarray, inputs: np.ndarray,
                 weights: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:  # fmt: skip
        template = self.template
        _native_op.check_optional(weights, template.weights, "weights")
        _native_op.check_optional(flags, template.flags, "flags")
        channels, baselines = vis.shape
        fn = template.instantiate(self.command_queue, channels, baselines, np.shape(gains)[-1])
        given = {"vis": vis, "gains": gains, "inputs": inputs, "weights": weights, "flags": flags}
        outputs = ["out_vis"] + (["out_weights"] if template.weights else []) + (
            ["out_flags"] if template.flags else [])  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, given, outputs)
        return (out[0], out[1] if template.weights else None,
                out[-1] if template.flags else None)  # fmt: skip


class SolveGainsTemplate(_native_op.NativeTemplate):
    """What produces the gains that :class:`ApplyGainsTemplate` applies: per channel, the
    per-input complex gains of a point source at the phase centre, solved with StEFCal from the
    ``vis``, ``weights`` and ``flags`` that :class:`.device.Finalise` leaves, in one kernel
    launch with one workgroup per channel; see :class:`host.SolveGainsHost` for every step.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    weights
        ``True``: there is a `weights` slot (every weight is 1 otherwise)
    flags
        ``True``: there is a `flags` slot
    initial
        ``True``: there is an `initial` slot with the gains to start from (1+0j otherwise)
    max_iterations, tol, reference, mask, corrections
        As for :class:`host.SolveGainsHost` (same errors)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.SolveGainsHost
    KERNEL = "ksp_solve_gains"

    def __init__(self, context: AbstractContext, weights: bool = True, flags: bool = True,
                 initial: bool = False, max_iterations: int = 30, tol: float = 1e-5,
                 reference: int = 0, mask: int = 0xFF, corrections: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.weights = bool(weights)
        self.flags = bool(flags)
        self.initial = bool(initial)
        checked = self.host_class(max_iterations, tol, reference, mask, corrections)
        self.max_iterations = checked.max_iterations
        self.tol = checked.tol
        self.tol2 = checked.tol2
        self.reference = checked.reference
        self.mask = checked.mask
        self.corrections = checked.corrections
        self._setup(context, tuning)


class SolveGains(_native_op.NativeOperation):
    """Concrete :class:`SolveGainsTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1, `n_inputs` outside 1..128 or the template's `reference` not below `n_inputs`).

    .. rubric:: Slots

    **vis** : channels x baselines, complex64
    **weights** : channels x baselines, float32 (only with ``weights``)
    **flags** : channels x baselines, uint8 (only with ``flags``)
    **pairs** : n_inputs x n_inputs, int32 (:meth:`host.SolveGainsHost.pair_table`)
    **initial** : channels x n_inputs, complex64 (only with ``initial``)
    **gains** : channels x n_inputs, complex64
    **iterations** : channels, int32
    **status** : channels, uint8

    Every padded dimension is an object of its own, so ``vis``, ``weights`` and ``flags`` can
    be compounded with :class:`.device.Finalise`'s outputs and ``gains`` with
    :class:`ApplyGains`'s ``gains``, each taking the other's padding. Binding one buffer to
    ``initial`` and ``gains`` refines the gains in place.
    """

    def __init__(self, template: SolveGainsTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self.n_inputs = template.host_class.check_n_inputs(n_inputs)
        if template.reference >= n_inputs:
            raise ValueError(f"reference must be -1 or 0..n_inputs-1 = {n_inputs - 1}, "
                             f"not {template.reference}")  # fmt: skip

        def samples(dtype) -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        def per_input() -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(n_inputs)), np.complex64)

        self.slots["vis"] = samples(np.complex64)
        if template.weights:
            self.slots["weights"] = samples(np.float32)
        if template.flags:
            self.slots["flags"] = samples(np.uint8)
        self.slots["pairs"] = accel.IOSlot(
            (accel.Dimension(n_inputs), accel.Dimension(n_inputs)), np.int32)  # fmt: skip
        if template.initial:
            self.slots["initial"] = per_input()
        self.slots["gains"] = per_input()
        self.slots["iterations"] = accel.IOSlot((accel.Dimension(channels),), np.int32)
        self.slots["status"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)

    def _arguments(self) -> list:
        """The arguments of ``ksp_solve_gains`` after ``(device, stream)``."""
        template = self.template
        vis, pairs, gains = self.buffer("vis"), self.buffer("pairs"), self.buffer("gains")
        weights = self.buffer("weights") if template.weights else None
        flags = self.buffer("flags") if template.flags else None
        initial = self.buffer("initial") if template.initial else None
        return [
            vis.buffer,
            _native_op.pointer(weights),
            _native_op.pointer(flags),
            pairs.buffer,
            _native_op.pointer(initial),
            gains.buffer,
            self.buffer("iterations").buffer,
            self.buffer("status").buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_inputs),
            np.int32(vis.padded_shape[1]),
            _native_op.stride(weights),
            _native_op.stride(flags),
            np.int32(pairs.padded_shape[1]),
            _native_op.stride(initial),
            np.int32(gains.padded_shape[1]),
            np.int32(template.max_iterations),
            np.float32(template.tol2),
            np.int32(template.reference),
            np.int32(template.mask),
            np.int32(template.corrections),
        ]

    def _run(self) -> None:
        self._launch(*self._arguments())

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(
            weights=template.weights, flags=template.flags, initial=template.initial,
            max_iterations=template.max_iterations, tol=template.tol,
            reference=template.reference, mask=template.mask, corrections=template.corrections,
            n_inputs=self.n_inputs)  # fmt: skip


SolveGainsTemplate.operation_class = SolveGains


class SolveGainsHostFromDevice:
    """Make a :class:`SolveGainsTemplate` callable like :class:`host.SolveGainsHost`, but with
    the ``inputs`` (baselines x 2) that :class:`ApplyGainsHostFromDevice` takes instead of the
    table, which it builds (:meth:`host.SolveGainsHost.pair_table`): ``(vis, inputs, n_inputs,
    weights=None, flags=None, initial=None)`` in, ``(gains, iterations, status)`` out; allocates
    on every call. ``TypeError`` unless `weights`, `flags` and `initial` are each given exactly
    when the template has them."""

    def __init__(self, template: SolveGainsTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis: np.ndarray, inputs: np.ndarray, n_inputs: int,
                 weights: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None,
                 initial: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:  # fmt: skip
        template = self.template
        _native_op.check_optional(weights, template.weights, "weights")
        _native_op.check_optional(flags, template.flags, "flags")
        _native_op.check_optional(initial, template.initial, "initial")
        channels, baselines = vis.shape
        if np.shape(inputs) != (baselines, 2):
            raise ValueError(f"inputs must have shape (baselines, 2) = ({baselines}, 2), "
                             f"not {np.shape(inputs)}")  # fmt: skip
        pairs = template.host_class.pair_table(inputs, n_inputs)
        fn = template.instantiate(self.command_queue, channels, baselines, n_inputs)
        given = {"vis": vis, "pairs": pairs, "weights": weights, "flags": flags,
                 "initial": initial}  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, given,
                                  ["gains", "iterations", "status"])  # fmt: skip
        return out[0], out[1], out[2]


class SolveGainsLargeTemplate(SolveGainsTemplate):
    """:class:`SolveGainsTemplate` for arrays of up to 512 inputs, with the same parameters
    (same errors, `reference` up to 511) and the same results; see
    :class:`host.SolveGainsLargeHost`. Above 128 inputs a channel's matrix does not fit LDS:
    a fixed grid of :attr:`SolveGainsLarge.WORKGROUPS` workgroups solves the channels one after
    another, each with its matrix in its own part of a work area in device memory. Up to 128
    inputs the operation is :class:`SolveGains` under another name: the same launcher, no work
    area.

    Parameters
    ----------
    tuning
        The launch geometry is fixed: nothing to tune, any key is a ``ValueError``
        (:func:`.tune.fixed_geometry`).
    """

    host_class = host.SolveGainsLargeHost
    KERNEL = "ksp_solve_gains_large"
    SMALL_KERNEL = SolveGainsTemplate.KERNEL

    def _setup(self, context: AbstractContext, tuning: Optional[Mapping[str, Any]]) -> None:
        super()._setup(context, tuning)
        self.small_kernel = context.native_kernel(self.SMALL_KERNEL)


class SolveGainsLarge(SolveGains):
    """Concrete :class:`SolveGainsLargeTemplate` (``ValueError`` if `channels` or `baselines`
    is below 1, `n_inputs` outside 1..512 or the template's `reference` not below `n_inputs`).

    .. rubric:: Slots

    Those of :class:`SolveGains`, which compound in the same way, and for `n_inputs` above 128

    **work_area** : :meth:`work_bytes` scratch bytes for the channels' matrices; exposed so
    that several operations that do not run at once can share one allocation (it need not be
    cleared)

    Up to 128 inputs there is no such slot and the launcher is that of :class:`SolveGains`.
    """

    #: the most inputs whose matrix the kernel of :class:`SolveGains` keeps in LDS
    SMALL_INPUTS = host.SolveGainsHost.MAX_INPUTS
    #: workgroups launched at most (``SGL_WORKGROUPS``): the parts of the work area
    WORKGROUPS = 256

    def __init__(self, template: SolveGainsLargeTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, n_inputs, allocator)
        if self.n_inputs > self.SMALL_INPUTS:
            self.slots["work_area"] = accel.IOSlot(
                (accel.Dimension(self.work_bytes(channels, n_inputs), exact=True),), np.uint8)  # fmt: skip

    @classmethod
    def work_bytes(cls, channels: int, n_inputs: int) -> int:
        """What ``ksp_solve_gains_large_work_bytes`` returns: for each of ``min(WORKGROUPS,
        channels)`` workgroups three float32 planes of `n_inputs` rows of `n_inputs` rounded up
        to 32 elements, at most 768 MiB; 0 up to 128 inputs and out of range."""
        if channels < 1 or not cls.SMALL_INPUTS < n_inputs <= host.SolveGainsLargeHost.MAX_INPUTS:
            return 0
        row = -(-n_inputs // 32) * 32
        return min(cls.WORKGROUPS, channels) * 3 * n_inputs * row * 4

    def _run(self) -> None:
        args = self._arguments()
        if self.n_inputs <= self.SMALL_INPUTS:
            self.command_queue.enqueue_kernel(self.template.small_kernel, args)
            return
        work = self.buffer("work_area")
        self._launch(*args[:8], work.buffer, np.uint64(work.shape[0]), *args[8:])


SolveGainsLargeTemplate.operation_class = SolveGainsLarge


class SolveGainsLargeHostFromDevice(SolveGainsHostFromDevice):
    """:class:`SolveGainsHostFromDevice` for a :class:`SolveGainsLargeTemplate`: the same
    arguments and results, `n_inputs` up to 512."""


class SolveJonesTemplate(_native_op.NativeTemplate):
    """The leakage solve beside :class:`SolveGainsTemplate`: per channel, one 2x2 Jones matrix
    per dual-feed antenna, solved with the full-polarisation StEFCal step from the ``vis``,
    ``weights`` and ``flags`` that :class:`.device.Finalise` (or :class:`Predict` with
    ``divide``) leaves, cross-hand baselines included, in one kernel launch with one workgroup
    per channel; see :class:`host.SolveJonesHost` for every step.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    weights
        ``True``: there is a `weights` slot (every weight is 1 otherwise)
    flags
        ``True``: there is a `flags` slot
    initial
        ``True``: there is an `initial` slot with the matrices to start from (the identity
        otherwise)
    max_iterations, tol, reference, mask, corrections
        As for :class:`host.SolveJonesHost` (same errors)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.SolveJonesHost
    KERNEL = "ksp_solve_jones"

    def __init__(self, context: AbstractContext, weights: bool = True, flags: bool = True,
                 initial: bool = False, max_iterations: int = 30, tol: float = 1e-5,
                 reference: int = 0, mask: int = 0xFF, corrections: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.weights = bool(weights)
        self.flags = bool(flags)
        self.initial = bool(initial)
        checked = host.SolveJonesHost(max_iterations, tol, reference, mask, corrections)
        self.max_iterations = checked.max_iterations
        self.tol = checked.tol
        self.tol2 = checked.tol2
        self.reference = checked.reference
        self.mask = checked.mask
        self.corrections = checked.corrections
        self._setup(context, tuning)


class SolveJones(_native_op.NativeOperation):
    """Concrete :class:`SolveJonesTemplate` (``ValueError`` if `channels` or `baselines` is
    below 1, `n_inputs` odd or outside 2..128, or the template's `reference` not below
    ``n_inputs / 2``).

    .. rubric:: Slots

    **vis** : channels x baselines, complex64
    **weights** : channels x baselines, float32 (only with ``weights``)
    **flags** : channels x baselines, uint8 (only with ``flags``)
    **pairs** : n_inputs x n_inputs, int32 (:meth:`host.SolveGainsHost.pair_table`)
    **initial** : channels x n_inputs x 2, complex64 (only with ``initial``)
    **jones** : channels x n_inputs x 2, complex64
    **iterations** : channels, int32
    **status** : channels, uint8

    Every padded dimension is an object of its own, so ``vis``, ``weights`` and ``flags`` can
    be compounded with :class:`.device.Finalise`'s or :class:`Predict`'s outputs, each taking
    the other's padding; the last axis of ``initial`` and ``jones`` is never padded. Binding
    one buffer to ``initial`` and ``jones`` refines the matrices in place.
    """

    def __init__(self, template: SolveJonesTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self.n_inputs = host.SolveJonesHost.check_n_inputs(n_inputs)
        if template.reference >= n_inputs // 2:
            raise ValueError(f"reference must be -1 or 0..n_inputs/2-1 = {n_inputs // 2 - 1}, "
                             f"not {template.reference}")  # fmt: skip

        def samples(dtype) -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        def per_input() -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(n_inputs),
                                 accel.Dimension(2, exact=True)), np.complex64)  # fmt: skip

        self.slots["vis"] = samples(np.complex64)
        if template.weights:
            self.slots["weights"] = samples(np.float32)
        if template.flags:
            self.slots["flags"] = samples(np.uint8)
        self.slots["pairs"] = accel.IOSlot(
            (accel.Dimension(n_inputs), accel.Dimension(n_inputs)), np.int32)  # fmt: skip
        if template.initial:
            self.slots["initial"] = per_input()
        self.slots["jones"] = per_input()
        self.slots["iterations"] = accel.IOSlot((accel.Dimension(channels),), np.int32)
        self.slots["status"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)

    def _run(self) -> None:
        template = self.template
        vis, pairs, jones = self.buffer("vis"), self.buffer("pairs"), self.buffer("jones")
        weights = self.buffer("weights") if template.weights else None
        flags = self.buffer("flags") if template.flags else None
        initial = self.buffer("initial") if template.initial else None
        self._launch(
            vis.buffer,
            _native_op.pointer(weights),
            _native_op.pointer(flags),
            pairs.buffer,
            _native_op.pointer(initial),
            jones.buffer,
            self.buffer("iterations").buffer,
            self.buffer("status").buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_inputs),
            np.int32(vis.padded_shape[1]),
            _native_op.stride(weights),
            _native_op.stride(flags),
            np.int32(pairs.padded_shape[1]),
            _native_op.stride(initial),
            np.int32(jones.padded_shape[1]),
            np.int32(template.max_iterations),
            np.float32(template.tol2),
            np.int32(template.reference),
            np.int32(template.mask),
            np.int32(template.corrections),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(
            weights=template.weights, flags=template.flags, initial=template.initial,
            max_iterations=template.max_iterations, tol=template.tol,
            reference=template.reference, mask=template.mask, corrections=template.corrections,
            n_inputs=self.n_inputs)  # fmt: skip


SolveJonesTemplate.operation_class = SolveJones


class SolveJonesHostFromDevice:
    """Make a :class:`SolveJonesTemplate` callable like :class:`host.SolveJonesHost`, but with
    the ``inputs`` (baselines x 2) that :class:`ApplyGainsHostFromDevice` takes instead of the
    table, which it builds (:meth:`host.SolveGainsHost.pair_table`): ``(vis, inputs, n_inputs,
    weights=None, flags=None, initial=None)`` in, ``(jones, iterations, status)`` out; allocates
    on every call. ``TypeError`` unless `weights`, `flags` and `initial` are each given exactly
    when the template has them."""

    def __init__(self, template: SolveJonesTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis: np.ndarray, inputs: np.ndarray, n_inputs: int,
                 weights: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None,
                 initial: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:  # fmt: skip
        template = self.template
        _native_op.check_optional(weights, template.weights, "weights")
        _native_op.check_optional(flags, template.flags, "flags")
        _native_op.check_optional(initial, template.initial, "initial")
        channels, baselines = vis.shape
        if np.shape(inputs) != (baselines, 2):
            raise ValueError(f"inputs must have shape (baselines, 2) = ({baselines}, 2), "
                             f"not {np.shape(inputs)}")  # fmt: skip
        pairs = host.SolveJonesHost.pair_table(inputs, n_inputs)
        fn = template.instantiate(self.command_queue, channels, baselines, n_inputs)
        given = {"vis": vis, "pairs": pairs, "weights": weights, "flags": flags,
                 "initial": initial}  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, given,
                                  ["jones", "iterations", "status"])  # fmt: skip
        return out[0], out[1], out[2]


class ApplyJonesTemplate(_native_op.NativeTemplate):
    """The step that closes the dual-polarisation chain: the per-antenna 2x2 matrices that
    :class:`SolveJonesTemplate` leaves with ``corrections=True`` applied to the ``vis`` that
    :class:`.device.Finalise` leaves, ``C_a V_ab C_b^H`` on the four products of every antenna
    pair, the ``weights`` propagated and the samples without a correction flagged, in one
    kernel launch; see :class:`host.ApplyJonesHost` for every step. The matrices are small
    (channels x inputs x 2) and stay on the device; only their application is per sample.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    weights
        ``True``: there are a `weights` and an `out_weights` slot
    flags
        ``True``: there are a `flags` and an `out_flags` slot
    flag_value
        As for :class:`host.ApplyJonesHost` (same errors)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.ApplyJonesHost
    KERNEL = "ksp_apply_jones"

    def __init__(self, context: AbstractContext, weights: bool = True, flags: bool = True,
                 flag_value: int = 128, tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.weights = bool(weights)
        self.flags = bool(flags)
        self.flag_value = host.ApplyJonesHost(flag_value).flag_value
        self._setup(context, tuning)


class ApplyJones(_native_op.NativeOperation):
    """Concrete :class:`ApplyJonesTemplate` (``ValueError`` if `channels`, `baselines` or
    `n_quads` is below 1 or `n_inputs` odd or outside 2..2048; ``TypeError`` if `n_inputs` or
    `n_quads` is not an integer).

    .. rubric:: Slots

    **vis**, **out_vis** : channels x baselines, complex64
    **weights**, **out_weights** : channels x baselines, float32 (only with ``weights``)
    **flags**, **out_flags** : channels x baselines, uint8 (only with ``flags``)
    **jones** : channels x n_inputs x 2, complex64: the matrices that multiply
    **quad_antennas** : n_quads x 2, int32, contiguous
    **quads** : n_quads x 4, int32, contiguous (:meth:`host.ApplyJonesHost.quad_table`)

    Every padded dimension is an object of its own, so ``jones`` can be compounded with
    :class:`SolveJones`' output, ``vis``, ``weights`` and ``flags`` with
    :class:`.device.Finalise`'s outputs and the ``out_*`` slots with the inputs of
    :class:`CompressWeights`, :class:`RangePercentiles` or the 2-D flagger, each taking the
    other's padding; the last axis of ``jones`` and of the two tables is never padded. Binding
    one buffer to ``vis`` and ``out_vis`` (and likewise to the other two pairs) applies the
    matrices in place; with buffers of their own the inputs are left untouched, and so are the
    output elements of a baseline that no quad names.
    """

    def __init__(self, template: ApplyJonesTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_inputs: int, n_quads: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self.n_inputs = host.ApplyJonesHost.check_n_inputs(n_inputs)
        if isinstance(n_quads, (bool, np.bool_)) or not isinstance(n_quads, (int, np.integer)):
            raise TypeError(f"n_quads {n_quads!r} is not an integer")
        if n_quads < 1:
            raise ValueError("n_quads must be at least 1")
        self.n_quads = int(n_quads)

        def pair(name: str, dtype) -> None:
            for slot in (name, "out_" + name):
                self.slots[slot] = accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        pair("vis", np.complex64)
        if template.weights:
            pair("weights", np.float32)
        if template.flags:
            pair("flags", np.uint8)
        self.slots["jones"] = accel.IOSlot(
            (channels, accel.Dimension(n_inputs), accel.Dimension(2, exact=True)), np.complex64)  # fmt: skip
        self.slots["quad_antennas"] = accel.IOSlot(
            (accel.Dimension(n_quads), accel.Dimension(2, exact=True)), np.int32)  # fmt: skip
        self.slots["quads"] = accel.IOSlot(
            (accel.Dimension(n_quads), accel.Dimension(4, exact=True)), np.int32)  # fmt: skip

    def _run(self) -> None:
        template = self.template
        vis, out_vis = self.buffer("vis"), self.buffer("out_vis")
        weights = self.buffer("weights") if template.weights else None
        out_weights = self.buffer("out_weights") if template.weights else None
        flags = self.buffer("flags") if template.flags else None
        out_flags = self.buffer("out_flags") if template.flags else None
        jones = self.buffer("jones")
        self._launch(
            vis.buffer,
            _native_op.pointer(weights),
            _native_op.pointer(flags),
            jones.buffer,
            self.buffer("quad_antennas").buffer,
            self.buffer("quads").buffer,
            out_vis.buffer,
            _native_op.pointer(out_weights),
            _native_op.pointer(out_flags),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_inputs),
            np.int32(self.n_quads),
            np.int32(vis.padded_shape[1]),
            _native_op.stride(weights),
            _native_op.stride(flags),
            np.int32(jones.padded_shape[1]),
            np.int32(out_vis.padded_shape[1]),
            _native_op.stride(out_weights),
            _native_op.stride(out_flags),
            np.int32(template.flag_value),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(weights=template.weights, flags=template.flags,
                                flag_value=template.flag_value, n_inputs=self.n_inputs,
                                n_quads=self.n_quads)  # fmt: skip


ApplyJonesTemplate.operation_class = ApplyJones


class ApplyJonesHostFromDevice:
    """Make an :class:`ApplyJonesTemplate` callable like :class:`host.ApplyJonesHost`, but with
    the ``inputs`` (baselines x 2) that :class:`SolveJonesHostFromDevice` takes instead of the
    table, which it builds (:meth:`host.ApplyJonesHost.quad_table`): ``(vis, jones, inputs,
    weights=None, flags=None)`` in, ``(out_vis, out_weights or None, out_flags or None)`` out;
    allocates on every call. The device outputs start as copies of the inputs, so a baseline
    that no quad names passes through, as with the host class. ``TypeError`` unless `weights`
    and `flags` are each given exactly when the template has them."""

    def __init__(self, template: ApplyJonesTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, vis: np.ndarray, jones: np.ndarray, inputs: np.ndarray,
                 weights: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:  # fmt: skip
        template = self.template
        _native_op.check_optional(weights, template.weights, "weights")
        _native_op.check_optional(flags, template.flags, "flags")
        channels, baselines = vis.shape
        if np.shape(inputs) != (baselines, 2):
            raise ValueError(f"inputs must have shape (baselines, 2) = ({baselines}, 2), "
                             f"not {np.shape(inputs)}")  # fmt: skip
        if np.ndim(jones) != 3:
            raise ValueError(f"jones must have shape (channels, n_inputs, 2), not {np.shape(jones)}")
        n_inputs = int(np.shape(jones)[1])
        quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, n_inputs)
        fn = template.instantiate(self.command_queue, channels, baselines, n_inputs, len(quads))
        given = {"vis": vis, "jones": jones, "quad_antennas": quad_antennas, "quads": quads,
                 "weights": weights, "flags": flags, "out_vis": vis, "out_weights": weights,
                 "out_flags": flags}  # fmt: skip
        outputs = ["out_vis"] + (["out_weights"] if template.weights else []) + (
            ["out_flags"] if template.flags else [])  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, given, outputs)
        return (out[0], out[1] if template.weights else None,
                out[-1] if template.flags else None)  # fmt: skip


class PredictTemplate(_native_op.NativeTemplate):
    """The step in front of :class:`SolveGainsTemplate` for a calibrator that is not a unit
    source at the phase centre: the model visibilities of up to 64 point sources evaluated per
    sample and, with `divide`, the ``vis`` that :class:`.device.Finalise` leaves divided by
    them, the ``weights`` scaled to match and the samples without a usable model flagged, in
    one kernel launch; see :class:`host.PredictHost` for every step.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    model
        ``True``: there is a `model` slot
    divide
        ``True``: there are a `vis` and an `out_vis` slot
    weights
        ``True``: with `divide`, there are a `weights` and an `out_weights` slot
    flags
        ``True``: with `divide`, there are a `flags` and an `out_flags` slot
    flag_value
        As for :class:`host.PredictHost` (same errors)
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).

    ``ValueError`` if neither `model` nor `divide` is set.
    """

    host_class = host.PredictHost
    KERNEL = "ksp_predict"

    def __init__(self, context: AbstractContext, model: bool = True, divide: bool = False,
                 weights: bool = True, flags: bool = True, flag_value: int = 64,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.model = bool(model)
        self.divide = bool(divide)
        if not (self.model or self.divide):
            raise ValueError("one of model and divide must be set")
        self.weights = self.divide and bool(weights)
        self.flags = self.divide and bool(flags)
        self.flag_value = host.PredictHost(flag_value).flag_value
        self._setup(context, tuning)


class Predict(_native_op.NativeOperation):
    """Concrete :class:`PredictTemplate` (``ValueError`` if `channels` or `baselines` is below
    1 or `n_sources` outside 1..64).

    .. rubric:: Slots

    **freqs** : channels, float64
    **delays** : n_sources x baselines, float64
    **flux** : channels x n_sources, float32
    **model** : channels x baselines, complex64 (only with ``model``)
    **vis**, **out_vis** : channels x baselines, complex64 (only with ``divide``)
    **weights**, **out_weights** : channels x baselines, float32 (only with ``weights``)
    **flags**, **out_flags** : channels x baselines, uint8 (only with ``flags``)

    Every padded dimension is an object of its own, so ``vis``, ``weights`` and ``flags`` can
    be compounded with :class:`.device.Finalise`'s outputs and the ``out_*`` slots with the
    inputs of :class:`SolveGains`, each taking the other's padding, while :class:`ApplyGains`
    keeps reading what :class:`.device.Finalise` left. Binding one buffer to ``vis`` and
    ``out_vis`` (and likewise to the other two pairs) divides in place.
    """

    def __init__(self, template: PredictTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_sources: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        if not 1 <= n_sources <= host.PredictHost.MAX_SOURCES:
            raise ValueError(f"n_sources must be 1..{host.PredictHost.MAX_SOURCES}")
        self.n_sources = n_sources

        def samples(dtype) -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

        self.slots["freqs"] = accel.IOSlot((accel.Dimension(channels),), np.float64)
        self.slots["delays"] = accel.IOSlot((n_sources, accel.Dimension(baselines)), np.float64)
        self.slots["flux"] = accel.IOSlot((channels, accel.Dimension(n_sources)), np.float32)
        if template.model:
            self.slots["model"] = samples(np.complex64)
        for name, present, dtype in (("vis", template.divide, np.complex64),
                                     ("weights", template.weights, np.float32),
                                     ("flags", template.flags, np.uint8)):  # fmt: skip
            if present:
                self.slots[name] = samples(dtype)
                self.slots["out_" + name] = samples(dtype)

    def _run(self) -> None:
        template = self.template

        def optional(name: str, present: bool) -> Optional[accel.DeviceArray]:
            return self.buffer(name) if present else None

        delays, flux = self.buffer("delays"), self.buffer("flux")
        model = optional("model", template.model)
        vis, out_vis = optional("vis", template.divide), optional("out_vis", template.divide)
        weights = optional("weights", template.weights)
        out_weights = optional("out_weights", template.weights)
        flags, out_flags = optional("flags", template.flags), optional("out_flags", template.flags)
        self._launch(
            self.buffer("freqs").buffer,
            delays.buffer,
            flux.buffer,
            _native_op.pointer(model),
            _native_op.pointer(vis),
            _native_op.pointer(weights),
            _native_op.pointer(flags),
            _native_op.pointer(out_vis),
            _native_op.pointer(out_weights),
            _native_op.pointer(out_flags),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_sources),
            np.int32(delays.padded_shape[1]),
            np.int32(flux.padded_shape[1]),
            _native_op.stride(model),
            _native_op.stride(vis),
            _native_op.stride(weights),
            _native_op.stride(flags),
            _native_op.stride(out_vis),
            _native_op.stride(out_weights),
            _native_op.stride(out_flags),
            np.int32(template.flag_value),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(model=template.model, divide=template.divide,
                                weights=template.weights, flags=template.flags,
                                flag_value=template.flag_value, n_sources=self.n_sources)  # fmt: skip


PredictTemplate.operation_class = Predict


class PredictHostFromDevice:
    """Make a :class:`PredictTemplate` callable like :class:`host.PredictHost`: ``(freqs,
    delays, flux, vis=None, weights=None, flags=None)`` in, ``(model or None, out_vis or None,
    out_weights or None, out_flags or None)`` out; allocates on every call. ``TypeError``
    unless `vis`, `weights` and `flags` are each given exactly when the template has them."""

    def __init__(self, template: PredictTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, freqs: np.ndarray, delays: np.ndarray, flux: np.ndarray,
                 vis: Optional[np.ndarray] = None, weights: Optional[np.ndarray] = None,
                 flags: Optional[np.ndarray] = None):  # fmt: skip
        template = self.template
        _native_op.check_optional(vis, template.divide, "vis")
        _native_op.check_optional(weights, template.weights, "weights")
        _native_op.check_optional(flags, template.flags, "flags")
        n_sources, baselines = np.shape(delays)
        fn = template.instantiate(self.command_queue, len(freqs), baselines, n_sources)
        given = {"freqs": freqs, "delays": delays, "flux": flux, "vis": vis, "weights": weights,
                 "flags": flags}  # fmt: skip
        present = {"model": template.model, "out_vis": template.divide,
                   "out_weights": template.weights, "out_flags": template.flags}  # fmt: skip
        names = [name for name, there in present.items() if there]
        out = dict(zip(names, _native_op.run_once(fn, self.command_queue, given, names)))
        return tuple(out.get(name) for name in present)


class FitDelaysTemplate(_native_op.NativeTemplate):
    """The first thing a pipeline does with the gains of :class:`SolveGainsTemplate`: per
    input, the delay and phase whose phasor best matches them across the band, and that
    smooth, unit-modulus phasor for every channel, the ones the solver lost included, which is
    what :class:`ApplyGainsTemplate` applies; one kernel launch with one workgroup per input;
    see :class:`host.FitDelaysHost` for every step.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    channel_width, n_fft, refine, status_mask, corrections
        As for :class:`host.FitDelaysHost` (same errors)
    status
        ``True``: there is a `status` slot (:class:`SolveGains`'s)
    model
        ``True``: there is a `model` slot
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.FitDelaysHost
    KERNEL = "ksp_fit_delays"

    def __init__(self, context: AbstractContext, channel_width: float,
                 n_fft: Optional[int] = None, refine: int = 3, status: bool = True,
                 status_mask: int = 0xFF, model: bool = True, corrections: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.checked = host.FitDelaysHost(channel_width, n_fft, refine, status_mask, corrections)
        self.channel_width = self.checked.channel_width
        self.n_fft = self.checked.n_fft
        self.refine = self.checked.refine
        self.status = bool(status)
        self.status_mask = self.checked.status_mask
        self.model = bool(model)
        self.corrections = self.checked.corrections
        self._setup(context, tuning)


class FitDelays(_native_op.NativeOperation):
    """Concrete :class:`FitDelaysTemplate` (``ValueError`` if `channels` is outside 1..8192,
    `n_inputs` below 1 or the template's `n_fft` below twice the channels).

    .. rubric:: Slots

    **gains** : channels x n_inputs, complex64
    **status** : channels, uint8 (only with ``status``)
    **delays** : n_inputs, float64
    **phasors** : n_inputs, complex64
    **amplitudes** : n_inputs, float32
    **fit_status** : n_inputs, uint8
    **model** : channels x n_inputs, complex64 (only with ``model``)

    Every padded dimension is an object of its own, so ``gains`` and ``status`` can be
    compounded with :class:`SolveGains`'s outputs and ``model`` with :class:`ApplyGains`'s
    ``gains``, each taking the other's padding.
    """

    def __init__(self, template: FitDelaysTemplate, command_queue: AbstractCommandQueue,
                 channels: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, n_inputs, allocator)
        self.n_inputs = n_inputs
        self.n_fft = template.checked.transform_length(channels, n_inputs)

        def per_input(dtype) -> accel.IOSlot:
            return accel.IOSlot((accel.Dimension(n_inputs),), dtype)

        def per_channel() -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(n_inputs)), np.complex64)

        self.slots["gains"] = per_channel()
        if template.status:
            self.slots["status"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)
        self.slots["delays"] = per_input(np.float64)
        self.slots["phasors"] = per_input(np.complex64)
        self.slots["amplitudes"] = per_input(np.float32)
        self.slots["fit_status"] = per_input(np.uint8)
        if template.model:
            self.slots["model"] = per_channel()

    def _run(self) -> None:
        template = self.template
        gains = self.buffer("gains")
        status = self.buffer("status") if template.status else None
        model = self.buffer("model") if template.model else None
        self._launch(
            gains.buffer,
            _native_op.pointer(status),
            self.buffer("delays").buffer,
            self.buffer("phasors").buffer,
            self.buffer("amplitudes").buffer,
            self.buffer("fit_status").buffer,
            _native_op.pointer(model),
            np.int32(self.channels),
            np.int32(self.n_inputs),
            np.int32(gains.padded_shape[1]),
            _native_op.stride(model),
            np.int32(self.n_fft),
            np.int32(template.refine),
            np.int32(template.status_mask),
            np.int32(template.corrections),
            np.float64(template.channel_width),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return {"channel_width": template.channel_width, "n_fft": self.n_fft,
                "refine": template.refine, "status": template.status,
                "status_mask": template.status_mask, "model": template.model,
                "corrections": template.corrections, "channels": self.channels,
                "n_inputs": self.n_inputs}  # fmt: skip


FitDelaysTemplate.operation_class = FitDelays


class FitDelaysHostFromDevice:
    """Make a :class:`FitDelaysTemplate` callable like :class:`host.FitDelaysHost`: ``(gains,
    status=None)`` in, ``(delays, phasors, amplitudes, fit_status, model or None)`` out;
    allocates on every call. ``TypeError`` unless `status` is given exactly when the template
    has it."""

    def __init__(self, template: FitDelaysTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, gains: np.ndarray, status: Optional[np.ndarray] = None):
        template = self.template
        _native_op.check_optional(status, template.status, "status")
        channels, n_inputs = np.shape(gains)
        fn = template.instantiate(self.command_queue, channels, n_inputs)
        names = ["delays", "phasors", "amplitudes", "fit_status"] + (
            ["model"] if template.model else [])  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, {"gains": gains, "status": status},
                                  names)  # fmt: skip
        return tuple(out) + (() if template.model else (None,))


class InterpolateGainsTemplate(_native_op.NativeTemplate):
    """What stands between :class:`SolveGainsTemplate` / :class:`FitDelaysTemplate` and the
    :class:`ApplyGainsTemplate` of a target scan: per input, the solved gains with the delay
    model divided out, smoothed, normalised, filled across the channels the solver left without
    a value (gaps of at most `max_gap` channels), multiplied by the delay model and by the
    band-wide gain of a later solve again, and inverted; one kernel launch with one workgroup
    per input; see :class:`host.InterpolateGainsHost` for every step.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    max_gap, smooth, normalise, status_mask, corrections
        As for :class:`host.InterpolateGainsHost` (same errors)
    status
        ``True``: there is a `status` slot (:class:`SolveGains`'s)
    model
        ``True``: there is a `model` slot (:class:`FitDelays`'s, fitted with
        ``corrections=False``)
    scale
        ``True``: there is a `scale` slot
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.InterpolateGainsHost
    KERNEL = "ksp_interpolate_gains"

    def __init__(self, context: AbstractContext, max_gap: int, smooth: int = 1,
                 normalise: bool = False, status: bool = True, status_mask: int = 0xFF,
                 model: bool = True, scale: bool = False, corrections: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.checked = host.InterpolateGainsHost(max_gap, smooth, normalise, status_mask,
                                                 corrections)  # fmt: skip
        self.max_gap = self.checked.max_gap
        self.smooth = self.checked.smooth
        self.normalise = self.checked.normalise
        self.status = bool(status)
        self.status_mask = self.checked.status_mask
        self.model = bool(model)
        self.scale = bool(scale)
        self.corrections = self.checked.corrections
        self._setup(context, tuning)


class InterpolateGains(_native_op.NativeOperation):
    """Concrete :class:`InterpolateGainsTemplate` (``ValueError`` if `channels` is outside
    1..16384 or `n_inputs` below 1).

    .. rubric:: Slots

    **gains** : channels x n_inputs, complex64
    **status** : channels, uint8 (only with ``status``)
    **model** : channels x n_inputs, complex64 (only with ``model``)
    **scale** : n_inputs, complex64 (only with ``scale``)
    **out** : channels x n_inputs, complex64
    **kept** : n_inputs, int32
    **filled** : n_inputs, int32
    **fill_status** : n_inputs, uint8
    **mean_amplitude** : n_inputs, float32 (only with ``normalise``)

    Every padded dimension is an object of its own, so ``gains`` and ``status`` can be
    compounded with :class:`SolveGains`'s outputs, ``model`` with :class:`FitDelays`'s and
    ``out`` with :class:`ApplyGains`'s ``gains``, each taking the other's padding. ``out`` may
    be bound to the buffer of ``gains``: the operation then works in place.
    """

    def __init__(self, template: InterpolateGainsTemplate, command_queue: AbstractCommandQueue,
                 channels: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, n_inputs, allocator)
        template.checked.check_shape(channels, n_inputs)
        self.n_inputs = n_inputs

        def per_input(dtype) -> accel.IOSlot:
            return accel.IOSlot((accel.Dimension(n_inputs),), dtype)

        def per_channel() -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(n_inputs)), np.complex64)

        self.slots["gains"] = per_channel()
        if template.status:
            self.slots["status"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)
        if template.model:
            self.slots["model"] = per_channel()
        if template.scale:
            self.slots["scale"] = per_input(np.complex64)
        self.slots["out"] = per_channel()
        self.slots["kept"] = per_input(np.int32)
        self.slots["filled"] = per_input(np.int32)
        self.slots["fill_status"] = per_input(np.uint8)
        if template.normalise:
            self.slots["mean_amplitude"] = per_input(np.float32)

    def _run(self) -> None:
        template = self.template
        gains = self.buffer("gains")
        status = self.buffer("status") if template.status else None
        model = self.buffer("model") if template.model else None
        scale = self.buffer("scale") if template.scale else None
        out = self.buffer("out")
        mean_amplitude = self.buffer("mean_amplitude") if template.normalise else None
        self._launch(
            gains.buffer,
            _native_op.pointer(status),
            _native_op.pointer(model),
            _native_op.pointer(scale),
            out.buffer,
            self.buffer("kept").buffer,
            self.buffer("filled").buffer,
            self.buffer("fill_status").buffer,
            _native_op.pointer(mean_amplitude),
            np.int32(self.channels),
            np.int32(self.n_inputs),
            np.int32(gains.padded_shape[1]),
            _native_op.stride(model),
            np.int32(out.padded_shape[1]),
            np.int32(template.max_gap),
            np.int32(template.smooth),
            np.int32(template.status_mask),
            np.int32(template.corrections),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return {"max_gap": template.max_gap, "smooth": template.smooth,
                "normalise": template.normalise, "status": template.status,
                "status_mask": template.status_mask, "model": template.model,
                "scale": template.scale, "corrections": template.corrections,
                "channels": self.channels, "n_inputs": self.n_inputs}  # fmt: skip


InterpolateGainsTemplate.operation_class = InterpolateGains


class InterpolateGainsHostFromDevice:
    """Make an :class:`InterpolateGainsTemplate` callable like
    :class:`host.InterpolateGainsHost`: ``(gains, status=None, model=None, scale=None)`` in,
    ``(out, kept, filled, fill_status, mean_amplitude or None)`` out; allocates on every call.
    ``TypeError`` unless `status`, `model` and `scale` are given exactly when the template has
    them."""

    def __init__(self, template: InterpolateGainsTemplate,
                 command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, gains: np.ndarray, status: Optional[np.ndarray] = None,
                 model: Optional[np.ndarray] = None, scale: Optional[np.ndarray] = None):  # fmt: skip
        template = self.template
        _native_op.check_optional(status, template.status, "status")
        _native_op.check_optional(model, template.model, "model")
        _native_op.check_optional(scale, template.scale, "scale")
        channels, n_inputs = np.shape(gains)
        fn = template.instantiate(self.command_queue, channels, n_inputs)
        names = ["out", "kept", "filled", "fill_status"] + (
            ["mean_amplitude"] if template.normalise else [])  # fmt: skip
        given = {"gains": gains, "status": status, "model": model, "scale": scale}
        out = _native_op.run_once(fn, self.command_queue, given, names)
        return tuple(out) + (() if template.normalise else (None,))


class InterpolateJonesTemplate(_native_op.NativeTemplate):
    """The 2x2 counterpart of :class:`InterpolateGainsTemplate`, between
    :class:`SolveJonesTemplate` (``corrections=False``) and the :class:`ApplyJonesTemplate` of
    a target scan: per antenna, the solved matrices with a delay model per feed divided out,
    smoothed, normalised, filled whole across the channels the solver left without a matrix
    (gaps of at most `max_gap` channels), multiplied by the model and by a band-wide gain per
    feed again, and inverted; one kernel launch with one workgroup per antenna; see
    :class:`host.InterpolateJonesHost` for every step. The `model` is what
    :class:`FitDelaysTemplate` (``corrections=False``) fits to the gains that
    :class:`JonesDiagonalTemplate` extracts.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    max_gap, smooth, normalise, status_mask, corrections
        As for :class:`host.InterpolateJonesHost` (same errors)
    status
        ``True``: there is a `status` slot (:class:`SolveJones`'s)
    model
        ``True``: there is a `model` slot (:class:`FitDelays`'s)
    scale
        ``True``: there is a `scale` slot
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.InterpolateJonesHost
    KERNEL = "ksp_interpolate_jones"

    def __init__(self, context: AbstractContext, max_gap: int, smooth: int = 1,
                 normalise: bool = False, status: bool = True, status_mask: int = 0xFF,
                 model: bool = True, scale: bool = False, corrections: bool = False,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.checked = host.InterpolateJonesHost(max_gap, smooth, normalise, status_mask,
                                                 corrections)  # fmt: skip
        self.max_gap = self.checked.max_gap
        self.smooth = self.checked.smooth
        self.normalise = self.checked.normalise
        self.status = bool(status)
        self.status_mask = self.checked.status_mask
        self.model = bool(model)
        self.scale = bool(scale)
        self.corrections = self.checked.corrections
        self._setup(context, tuning)


class InterpolateJones(_native_op.NativeOperation):
    """Concrete :class:`InterpolateJonesTemplate` (``ValueError`` if `channels` is outside
    1..16384 or `n_inputs` is odd or outside 2..2048).

    .. rubric:: Slots

    **jones** : channels x n_inputs x 2, complex64 (the last axis is not padded)
    **status** : channels, uint8 (only with ``status``)
    **model** : channels x n_inputs, complex64 (only with ``model``)
    **scale** : n_inputs, complex64 (only with ``scale``)
    **out** : channels x n_inputs x 2, complex64 (the last axis is not padded)
    **kept** : n_inputs // 2, int32
    **filled** : n_inputs // 2, int32
    **fill_status** : n_inputs // 2, uint8
    **mean_amplitude** : n_inputs // 2, float32 (only with ``normalise``)

    Every padded dimension is an object of its own, so ``jones`` and ``status`` can be
    compounded with :class:`SolveJones`'s outputs, ``model`` with :class:`FitDelays`'s and
    ``out`` with :class:`ApplyJones`'s ``jones``, each taking the other's padding. ``out`` may
    be bound to the buffer of ``jones``: the operation then works in place.
    """

    def __init__(self, template: InterpolateJonesTemplate, command_queue: AbstractCommandQueue,
                 channels: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, n_inputs, allocator)
        template.checked.check_shape(channels, n_inputs)
        self.n_inputs = n_inputs

        def per_antenna(dtype) -> accel.IOSlot:
            return accel.IOSlot((accel.Dimension(n_inputs // 2),), dtype)

        def matrices() -> accel.IOSlot:
            return accel.IOSlot((channels, accel.Dimension(n_inputs),
                                 accel.Dimension(2, exact=True)), np.complex64)  # fmt: skip

        self.slots["jones"] = matrices()
        if template.status:
            self.slots["status"] = accel.IOSlot((accel.Dimension(channels),), np.uint8)
        if template.model:
            self.slots["model"] = accel.IOSlot((channels, accel.Dimension(n_inputs)),
                                               np.complex64)  # fmt: skip
        if template.scale:
            self.slots["scale"] = accel.IOSlot((accel.Dimension(n_inputs),), np.complex64)
        self.slots["out"] = matrices()
        self.slots["kept"] = per_antenna(np.int32)
        self.slots["filled"] = per_antenna(np.int32)
        self.slots["fill_status"] = per_antenna(np.uint8)
        if template.normalise:
            self.slots["mean_amplitude"] = per_antenna(np.float32)

    def _run(self) -> None:
        template = self.template
        jones = self.buffer("jones")
        status = self.buffer("status") if template.status else None
        model = self.buffer("model") if template.model else None
        scale = self.buffer("scale") if template.scale else None
        out = self.buffer("out")
        mean_amplitude = self.buffer("mean_amplitude") if template.normalise else None
        self._launch(
            jones.buffer,
            _native_op.pointer(status),
            _native_op.pointer(model),
            _native_op.pointer(scale),
            out.buffer,
            self.buffer("kept").buffer,
            self.buffer("filled").buffer,
            self.buffer("fill_status").buffer,
            _native_op.pointer(mean_amplitude),
            np.int32(self.channels),
            np.int32(self.n_inputs),
            np.int32(jones.padded_shape[1]),
            _native_op.stride(model),
            np.int32(out.padded_shape[1]),
            np.int32(template.max_gap),
            np.int32(template.smooth),
            np.int32(template.status_mask),
            np.int32(template.corrections),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return {"max_gap": template.max_gap, "smooth": template.smooth,
                "normalise": template.normalise, "status": template.status,
                "status_mask": template.status_mask, "model": template.model,
                "scale": template.scale, "corrections": template.corrections,
                "channels": self.channels, "n_inputs": self.n_inputs}  # fmt: skip


InterpolateJonesTemplate.operation_class = InterpolateJones


class InterpolateJonesHostFromDevice:
    """Make an :class:`InterpolateJonesTemplate` callable like
    :class:`host.InterpolateJonesHost`: ``(jones, status=None, model=None, scale=None)`` in,
    ``(out, kept, filled, fill_status, mean_amplitude or None)`` out; allocates on every call.
    ``TypeError`` unless `status`, `model` and `scale` are given exactly when the template has
    them."""

    def __init__(self, template: InterpolateJonesTemplate,
                 command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, jones: np.ndarray, status: Optional[np.ndarray] = None,
                 model: Optional[np.ndarray] = None, scale: Optional[np.ndarray] = None):  # fmt: skip
        template = self.template
        _native_op.check_optional(status, template.status, "status")
        _native_op.check_optional(model, template.model, "model")
        _native_op.check_optional(scale, template.scale, "scale")
        channels, n_inputs = np.shape(jones)[:2]
        fn = template.instantiate(self.command_queue, channels, n_inputs)
        names = ["out", "kept", "filled", "fill_status"] + (
            ["mean_amplitude"] if template.normalise else [])  # fmt: skip
        given = {"jones": jones, "status": status, "model": model, "scale": scale}
        out = _native_op.run_once(fn, self.command_queue, given, names)
        return tuple(out) + (() if template.normalise else (None,))


class JonesDiagonalTemplate(_native_op.NativeTemplate):
    """The diagonal of every antenna's 2x2 matrix as per-input gains, ``gains[c, p] = jones[c,
    p, p % 2]``: what lets :class:`FitDelaysTemplate` fit one delay per feed to the table of
    :class:`SolveJonesTemplate`; see :class:`host.JonesDiagonalHost`. One kernel launch.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    tuning
        Nothing to tune, any key is a ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.JonesDiagonalHost
    KERNEL = "ksp_jones_diagonal"

    def __init__(self, context: AbstractContext,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:
        self._setup(context, tuning)


class JonesDiagonal(_native_op.NativeOperation):
    """Concrete :class:`JonesDiagonalTemplate` (``ValueError`` if `channels` or `n_inputs` is
    below 1).

    .. rubric:: Slots

    **jones** : channels x n_inputs x 2, complex64 (the last axis is not padded)
    **gains** : channels x n_inputs, complex64

    Every padded dimension is an object of its own: ``jones`` compounds with
    :class:`SolveJones`'s output and ``gains`` with :class:`FitDelays`'s input.
    """

    def __init__(self, template: JonesDiagonalTemplate, command_queue: AbstractCommandQueue,
                 channels: int, n_inputs: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, n_inputs, allocator)
        if channels < 1:
            raise ValueError("channels must be at least 1")
        if n_inputs < 1:
            raise ValueError("n_inputs must be at least 1")
        self.n_inputs = n_inputs
        self.slots["jones"] = accel.IOSlot(
            (channels, accel.Dimension(n_inputs), accel.Dimension(2, exact=True)), np.complex64)  # fmt: skip
        self.slots["gains"] = accel.IOSlot((channels, accel.Dimension(n_inputs)), np.complex64)

    def _run(self) -> None:
        jones, gains = self.buffer("jones"), self.buffer("gains")
        self._launch(
            jones.buffer,
            gains.buffer,
            np.int32(self.channels),
            np.int32(self.n_inputs),
            np.int32(jones.padded_shape[1]),
            np.int32(gains.padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        return {"channels": self.channels, "n_inputs": self.n_inputs}


JonesDiagonalTemplate.operation_class = JonesDiagonal


class JonesDiagonalHostFromDevice:
    """Make a :class:`JonesDiagonalTemplate` callable like :class:`host.JonesDiagonalHost`:
    ``(jones)`` in, ``gains`` out; allocates on every call."""

    def __init__(self, template: JonesDiagonalTemplate,
                 command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, jones: np.ndarray) -> np.ndarray:
        channels, n_inputs = np.shape(jones)[:2]
        fn = self.template.instantiate(self.command_queue, channels, n_inputs)
        return _native_op.run_once(fn, self.command_queue, {"jones": jones}, ["gains"])[0]


class RangePercentilesTemplate(_native_op.NativeTemplate):
    """The step that closes the chain: the signal-display product of the ``vis`` and ``flags``
    that :class:`.device.Finalise` (or the flagger) leaves. For every range of baselines and
    every channel, the 0/100/25/75/50 % amplitudes of the samples that are neither NaN nor
    flagged under `mask`, the number of those samples and the OR of the range's flags: every
    range in one kernel launch; see :class:`host.RangePercentilesHost` for every step. With
    nothing left out, the five rows of a range are what :class:`..percentile.Percentile5` gives
    for that ``column_range``.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    is_amplitude
        ``True``: `data` is float32 amplitudes (non-negative with the sign bit clear, or NaN);
        ``False``: complex64
    use_flags
        ``True``: there are a `flags` and a `range_flags` slot
    mask
        As for :class:`host.RangePercentilesHost` (same errors); ``ValueError`` if it is not 0
        and `use_flags` is false
    tuning
        The kernel picks its launch geometry from the ranges: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.RangePercentilesHost
    KERNEL = "ksp_range_percentiles"

    def __init__(self, context: AbstractContext, is_amplitude: bool = False,
                 use_flags: bool = True, mask: int = 0,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.is_amplitude = bool(is_amplitude)
        self.use_flags = bool(use_flags)
        self.mask = host.check_mask_byte("mask", mask)
        if self.mask != 0 and not self.use_flags:
            raise ValueError(f"mask {self.mask:#x} needs use_flags")
        self._setup(context, tuning)


class RangePercentiles(_native_op.NativeOperation):
    """Concrete :class:`RangePercentilesTemplate` (``ValueError`` if `channels` or `baselines`
    is below 1, or for `ranges` that :func:`host.check_ranges` rejects for `baselines`).

    .. rubric:: Slots

    **data** : channels x baselines, float32 (``is_amplitude``) or complex64
    **flags** : channels x baselines, uint8 (only with ``use_flags``)
    **percentiles** : n_ranges x 5 x channels, float32, rows [0, 100, 25, 75, 50] %
    **counts** : n_ranges x channels, uint32
    **range_flags** : n_ranges x channels, uint8 (only with ``use_flags``)

    Every padded dimension is an object of its own, so ``data`` and ``flags`` can be
    compounded with :class:`.device.Finalise`'s ``vis`` and ``flags`` (or the flagger's) and
    take their padding.
    """

    def __init__(self, template: RangePercentilesTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, ranges,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self.ranges = host.check_ranges(ranges, baselines)
        n_ranges = len(self.ranges)
        # a host array the launcher copies during the call
        self._ranges = (ctypes.c_int * (2 * n_ranges))(*[v for pair in self.ranges for v in pair])

        def exact(size: int) -> accel.Dimension:
            return accel.Dimension(size, exact=True)

        dtype = np.float32 if template.is_amplitude else np.complex64
        self.slots["data"] = accel.IOSlot((channels, accel.Dimension(baselines)), dtype)
        if template.use_flags:
            self.slots["flags"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.uint8)
        self.slots["percentiles"] = accel.IOSlot(
            (exact(n_ranges), exact(5), accel.Dimension(channels)), np.float32)  # fmt: skip
        self.slots["counts"] = accel.IOSlot(
            (exact(n_ranges), accel.Dimension(channels)), np.uint32)  # fmt: skip
        if template.use_flags:
            self.slots["range_flags"] = accel.IOSlot(
                (exact(n_ranges), accel.Dimension(channels)), np.uint8)  # fmt: skip

    def _run(self) -> None:
        template = self.template
        data, percentiles, counts = (self.buffer(name) for name in ("data", "percentiles", "counts"))
        flags = self.buffer("flags") if template.use_flags else None
        range_flags = self.buffer("range_flags") if template.use_flags else None
        self._launch(
            data.buffer,
            _native_op.pointer(flags),
            percentiles.buffer,
            counts.buffer,
            _native_op.pointer(range_flags),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(data.padded_shape[1]),
            _native_op.stride(flags),
            np.int32(percentiles.padded_shape[2]),
            np.int32(counts.padded_shape[1]),
            _native_op.stride(range_flags),
            self._ranges,
            np.int32(len(self.ranges)),
            np.int32(template.is_amplitude),
            np.int32(template.mask),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(
            is_amplitude=template.is_amplitude,
            use_flags=template.use_flags,
            mask=template.mask,
            ranges=[list(pair) for pair in self.ranges],
        )


RangePercentilesTemplate.operation_class = RangePercentiles


class RangePercentilesHostFromDevice:
    """Make a :class:`RangePercentilesTemplate` callable like
    :class:`host.RangePercentilesHost`: ``(data, flags=None)`` in, ``(percentiles, counts,
    range_flags or None)`` out; allocates on every call. ``TypeError`` unless `flags` is given
    exactly when the template has ``use_flags``."""

    def __init__(self, template: RangePercentilesTemplate, command_queue: AbstractCommandQueue,
                 ranges) -> None:  # fmt: skip
        self.template = template
        self.command_queue = command_queue
        self.ranges = host.check_ranges(ranges)

    def __call__(self, data: np.ndarray, flags: Optional[np.ndarray] = None
                 ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:  # fmt: skip
        template = self.template
        _native_op.check_optional(flags, template.use_flags, "flags")
        channels, baselines = data.shape
        fn = template.instantiate(self.command_queue, channels, baselines, self.ranges)
        outputs = ["percentiles", "counts"] + (["range_flags"] if template.use_flags else [])
        out = _native_op.run_once(fn, self.command_queue, {"data": data, "flags": flags}, outputs)
        return out[0], out[1], (out[2] if template.use_flags else None)


class BandAverageTemplate(_native_op.NativeTemplate):
    """The other display product of the ``vis`` and ``flags`` that :class:`.device.Finalise`
    (or the flagger) leaves, the "time series": for every baseline and each of up to 8 series
    of channel weights, the weighted mean of the visibility and of its amplitude over the
    channels whose samples are neither NaN nor flagged under `mask`, the weight sum, the number
    of samples kept and the OR of the flags of the series' channels. Every sample is read from
    memory once, however many series there are; see :class:`host.BandAverageHost` for every
    step.

    Parameters
    ----------
    context
        Context whose device will run the kernels
    use_flags
        ``True``: there are a `flags` and a `series_flags` slot
    mask
        As for :class:`host.BandAverageHost` (same errors); ``ValueError`` if it is not 0 and
        `use_flags` is false
    tuning
        The launcher picks its launch geometry from the shape, and the block of the sums is
        part of the definition: nothing to tune, any key is a ``ValueError``
        (:func:`.tune.fixed_geometry`).
    """

    host_class = host.BandAverageHost
    KERNEL = "ksp_band_average"

    def __init__(self, context: AbstractContext, use_flags: bool = True, mask: int = 0,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        self.use_flags = bool(use_flags)
        self.mask = host.check_mask_byte("mask", mask)
        if self.mask != 0 and not self.use_flags:
            raise ValueError(f"mask {self.mask:#x} needs use_flags")
        self._setup(context, tuning)


class BandAverage(_native_op.NativeOperation):
    """Concrete :class:`BandAverageTemplate` (``ValueError`` unless `channels` is 1..262144,
    `baselines` at least 1 and `n_series` 1..8).

    .. rubric:: Slots

    **data** : channels x baselines, complex64
    **flags** : channels x baselines, uint8 (only with ``use_flags``)
    **channel_weights** : n_series x channels, float32
    **mean** : n_series x baselines, complex64
    **mean_amplitude** : n_series x baselines, float32
    **weight_sums** : n_series x baselines, float32
    **counts** : n_series x baselines, uint32
    **series_flags** : n_series x baselines, uint8 (only with ``use_flags``)
    **work_area** : :meth:`work_bytes` scratch bytes for the partial sums of the blocks of
    channels; exposed so that several operations that do not run at once can share one
    allocation (it need not be cleared)

    Every padded dimension is an object of its own, so ``data`` and ``flags`` can be
    compounded with :class:`.device.Finalise`'s ``vis`` and ``flags`` (or the flagger's) and
    take their padding.
    """

    def __init__(self, template: BandAverageTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int, n_series: int = 1,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if not 1 <= channels <= host.BandAverageHost.MAX_CHANNELS or baselines < 1:
            raise ValueError("channels must be 1..262144 and baselines at least 1")
        if not 1 <= n_series <= host.BandAverageHost.MAX_SERIES:
            raise ValueError(f"n_series must be 1..{host.BandAverageHost.MAX_SERIES}")
        self.n_series = n_series

        def series(dtype) -> accel.IOSlot:
            return accel.IOSlot(
                (accel.Dimension(n_series, exact=True), accel.Dimension(baselines)), dtype)  # fmt: skip

        self.slots["data"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.complex64)
        if template.use_flags:
            self.slots["flags"] = accel.IOSlot((channels, accel.Dimension(baselines)), np.uint8)
        self.slots["channel_weights"] = accel.IOSlot(
            (accel.Dimension(n_series, exact=True), accel.Dimension(channels)), np.float32)  # fmt: skip
        self.slots["mean"] = series(np.complex64)
        self.slots["mean_amplitude"] = series(np.float32)
        self.slots["weight_sums"] = series(np.float32)
        self.slots["counts"] = series(np.uint32)
        if template.use_flags:
            self.slots["series_flags"] = series(np.uint8)
        self.slots["work_area"] = accel.IOSlot(
            (accel.Dimension(self.work_bytes(channels, baselines, n_series), exact=True),), np.uint8)  # fmt: skip

    @staticmethod
    def work_bytes(channels: int, baselines: int, n_series: int) -> int:
        """What ``ksp_band_average_work_bytes`` returns: five 4-byte words per block of
        channels, series and baseline."""
        n_blocks = -(-channels // host.BandAverageHost.BLOCK)
        return n_blocks * n_series * 5 * baselines * 4

    def _run(self) -> None:
        template = self.template
        names = ("data", "channel_weights", "mean", "mean_amplitude", "weight_sums", "counts")
        data, weights, mean, amplitude, sums, counts = (self.buffer(name) for name in names)
        flags = self.buffer("flags") if template.use_flags else None
        series_flags = self.buffer("series_flags") if template.use_flags else None
        work = self.buffer("work_area")
        self._launch(
            data.buffer,
            _native_op.pointer(flags),
            weights.buffer,
            mean.buffer,
            amplitude.buffer,
            sums.buffer,
            counts.buffer,
            _native_op.pointer(series_flags),
            work.buffer,
            np.uint64(work.shape[0]),
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(self.n_series),
            np.int32(data.padded_shape[1]),
            _native_op.stride(flags),
            np.int32(weights.padded_shape[1]),
            np.int32(mean.padded_shape[1]),
            np.int32(amplitude.padded_shape[1]),
            np.int32(sums.padded_shape[1]),
            np.int32(counts.padded_shape[1]),
            _native_op.stride(series_flags),
            np.int32(template.mask),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(
            use_flags=template.use_flags, mask=template.mask, n_series=self.n_series)  # fmt: skip


BandAverageTemplate.operation_class = BandAverage


class BandAverageHostFromDevice:
    """Make a :class:`BandAverageTemplate` callable like :class:`host.BandAverageHost`:
    ``(data, channel_weights, flags=None)`` in, ``(mean, mean_amplitude, weight_sums, counts,
    series_flags or None)`` out; allocates on every call. ``TypeError`` unless `flags` is
    given exactly when the template has ``use_flags``."""

    def __init__(self, template: BandAverageTemplate, command_queue: AbstractCommandQueue) -> None:
        self.template = template
        self.command_queue = command_queue

    def __call__(self, data: np.ndarray, channel_weights: np.ndarray,
                 flags: Optional[np.ndarray] = None):  # fmt: skip
        template = self.template
        _native_op.check_optional(flags, template.use_flags, "flags")
        channels, baselines = data.shape
        fn = template.instantiate(self.command_queue, channels, baselines, channel_weights.shape[0])
        inputs = {"data": data, "channel_weights": channel_weights, "flags": flags}
        outputs = ["mean", "mean_amplitude", "weight_sums", "counts"] + (
            ["series_flags"] if template.use_flags else [])  # fmt: skip
        out = _native_op.run_once(fn, self.command_queue, inputs, outputs)
        return out[0], out[1], out[2], out[3], (out[4] if template.use_flags else None)


#: the most dumps one :class:`AccumulateBlock` launch adds
MAX_DUMPS = 8


class AccumulateBlockTemplate(_native_op.NativeTemplate):
    """Add a block of up to `dumps` dumps to the accumulators of :class:`.device.Accumulate`
    and :class:`.device.Finalise` in one kernel launch. For every sample the steps of
    :meth:`host.AveragerHost.add` run on dump 0, then on dump 1 and so on, so the result is
    bit for bit what as many launches of :class:`.device.Accumulate` leave, in that order;
    but the accumulators, 26 of the 39 bytes a sample costs per dump, are read and written
    once per block: 13 D + 26 bytes per sample for D dumps instead of 39 D.

    Parameters
    ----------
    context
        Context whose device will run the kernel
    dumps
        The most dumps a launch adds, 1 .. :data:`MAX_DUMPS` (``ValueError``): the operation
        has that many sets of input slots
    use_weights, input_flags
        As for :class:`.device.AccumulateTemplate`
    tuning
        The kernel picks its launch geometry from the shape: nothing to tune, any key is a
        ``ValueError`` (:func:`.tune.fixed_geometry`).
    """

    host_class = host.AveragerHost
    KERNEL = "ksp_average_accumulate_block"

    def __init__(self, context: AbstractContext, dumps: int, use_weights: bool = True,
                 input_flags: host.BackgroundFlags = host.BackgroundFlags.NONE,
                 tuning: Optional[Mapping[str, Any]] = None) -> None:  # fmt: skip
        if not 1 <= dumps <= MAX_DUMPS:
            raise ValueError(f"dumps must be 1..{MAX_DUMPS}")
        self.dumps = int(dumps)
        self.use_weights = bool(use_weights)
        self.input_flags = host.BackgroundFlags(input_flags)
        self._setup(context, tuning)


class AccumulateBlock(_native_op.NativeOperation):
    """Concrete :class:`AccumulateBlockTemplate` (``ValueError`` if `channels` or `baselines`
    is below 1). D stands for the template's `dumps`.

    .. rubric:: Slots

    **vis0** .. **vis{D-1}** : channels x baselines, complex64
    **flags0** .. **flags{D-1}** : channels x baselines, uint8 (any non-zero byte means flagged)
    **weights0** .. **weights{D-1}** : channels x baselines, float32 (only with ``use_weights``)
    **input_flags0** .. **input_flags{D-1}** : channels x baselines, uint8 (only in FULL mode)
    **input_flags** : channels, uint8 (only in CHANNEL mode: one mask for the block)
    **acc_vis** : channels x baselines, complex64
    **acc_weights** : channels x baselines, float32
    **acc_flags** : channels x baselines, uint8

    The kernel takes one row stride per kind, so the slots of one kind share one dimension
    object for the baselines and get one padded size; each kind, and each accumulator, has a
    dimension of its own. Every per-dump slot can so be compounded with the ``vis``,
    ``input_flags`` or ``weights`` of a :class:`Prepare`, with the fused flagger's ``vis`` or
    ``flags``, and the accumulators with :class:`.device.Finalise`'s.

    :attr:`n_dumps`, the number of dumps the next call adds, starts at D and can be set to
    1 .. D (``ValueError``) for the short block at the end of an integration. A call uses, and
    allocates if need be, only the slots of the first `n_dumps` dumps.
    """

    def __init__(self, template: AccumulateBlockTemplate, command_queue: AbstractCommandQueue,
                 channels: int, baselines: int,
                 allocator: Optional[AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(template, command_queue, channels, baselines, allocator)
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        self._n_dumps = template.dumps

        def per_dump(kind: str, dtype) -> None:
            dim = accel.Dimension(baselines)
            for d in range(template.dumps):
                self.slots[f"{kind}{d}"] = accel.IOSlot((channels, dim), dtype)

        per_dump("vis", np.complex64)
        per_dump("flags", np.uint8)
        if template.use_weights:
            per_dump("weights", np.float32)
        if template.input_flags == host.BackgroundFlags.FULL:
            per_dump("input_flags", np.uint8)
        elif template.input_flags == host.BackgroundFlags.CHANNEL:
            self.slots["input_flags"] = accel.IOSlot((channels,), np.uint8)
        for name, dtype in (("acc_vis", np.complex64), ("acc_weights", np.float32),
                            ("acc_flags", np.uint8)):  # fmt: skip
            self.slots[name] = accel.IOSlot((channels, accel.Dimension(baselines)), dtype)

    @property
    def n_dumps(self) -> int:
        return self._n_dumps

    @n_dumps.setter
    def n_dumps(self, value: int) -> None:
        if not 1 <= value <= self.template.dumps:
            raise ValueError(f"n_dumps must be 1..{self.template.dumps}")
        self._n_dumps = int(value)

    def _used(self, name: str) -> bool:
        """Whether a call with the present `n_dumps` touches slot `name`."""
        digits = name.lstrip("abcdefghijklmnopqrstuvwxyz_")
        return not digits or int(digits) < self._n_dumps

    def ensure_all_bound(self) -> None:
        for name, slot in self.slots.items():
            if self._used(name) and not slot.is_bound():
                slot.allocate(self.allocator)

    def _dumps(self, kind: str) -> List[accel.DeviceArray]:
        return [self.buffer(f"{kind}{d}") for d in range(self._n_dumps)]

    @staticmethod
    def _pointers(buffers: Optional[Sequence[accel.DeviceArray]]):
        """The host array of device pointers the launcher reads during the call (None for
        optional dumps that are absent)."""
        if buffers is None:
            return None
        return (ctypes.c_void_p * len(buffers))(*[b.buffer.ptr for b in buffers])

    def _run(self) -> None:
        template = self.template
        mode = template.input_flags
        full = mode == host.BackgroundFlags.FULL
        vis, flags = self._dumps("vis"), self._dumps("flags")
        weights = self._dumps("weights") if template.use_weights else None
        if full:
            in_flags = self._dumps("input_flags")
        elif mode:
            in_flags = [self.buffer("input_flags")] * self._n_dumps
        else:
            in_flags = None
        acc = [self.buffer(name) for name in ("acc_vis", "acc_weights", "acc_flags")]
        self._launch(
            np.int32(self._n_dumps),
            self._pointers(vis),
            self._pointers(flags),
            self._pointers(weights),
            self._pointers(in_flags),
            np.int32(mode.value),
            acc[0].buffer,
            acc[1].buffer,
            acc[2].buffer,
            np.int32(self.channels),
            np.int32(self.baselines),
            np.int32(vis[0].padded_shape[1]),
            np.int32(flags[0].padded_shape[1]),
            np.int32(weights[0].padded_shape[1] if weights is not None else 0),
            np.int32(in_flags[0].padded_shape[1] if full else 0),
            np.int32(acc[0].padded_shape[1]),
            np.int32(acc[1].padded_shape[1]),
            np.int32(acc[2].padded_shape[1]),
        )

    def parameters(self) -> Mapping[str, Any]:
        template = self.template
        return self._parameters(dumps=template.dumps, use_weights=template.use_weights,
                                input_flags=template.input_flags.name)  # fmt: skip


AccumulateBlockTemplate.operation_class = AccumulateBlock


class BlockAveragerHostFromDevice:
    """Present an :class:`AccumulateBlockTemplate` and a :class:`.device.FinaliseTemplate`
    like :class:`host.AveragerHost`, a block at a time: :meth:`add_block` takes sequences of
    1 .. `dumps` arrays and does what as many calls of ``add`` do, :meth:`finalise` is the host
    class's. The operations are instantiated and the shared accumulators allocated and zeroed
    once, here; with a `finalise_template` built with ``clear=False`` the accumulators keep
    their sums across :meth:`finalise`, unlike the host class."""

    def __init__(self, block_template: AccumulateBlockTemplate, finalise_template,
                 command_queue: AbstractCommandQueue, channels: int, baselines: int) -> None:  # fmt: skip
        self.command_queue = command_queue
        self.input_flags = block_template.input_flags
        self.use_weights = block_template.use_weights
        self.dumps = block_template.dumps
        self._block = block_template.instantiate(command_queue, channels, baselines)
        self._finalise = finalise_template.instantiate(command_queue, channels, baselines)
        shared = ("acc_vis", "acc_weights", "acc_flags")
        self._sequence = accel.OperationSequence(
            command_queue, [("block", self._block), ("finalise", self._finalise)],
            compounds={name: ["block:" + name, "finalise:" + name] for name in shared})
        for name in shared:
            self._sequence.ensure_bound(name)
            self._sequence.buffer(name).zero(command_queue)

    def add_block(self, vis: Sequence[np.ndarray], flags: Sequence[np.ndarray],
                  weights: Optional[Sequence[Optional[np.ndarray]]] = None,
                  input_flags: Optional[Sequence[np.ndarray]] = None) -> None:  # fmt: skip
        """Add ``len(vis)`` dumps. `weights` is a sequence of that length (an entry of None:
        weights of 1 for that dump) or None (1 for all); ``TypeError`` if it is given and the
        template has no weights. `input_flags` is a sequence of that length exactly when the
        template has a mask (``TypeError``); in CHANNEL mode the block has one mask, so its
        entries must be equal (``ValueError``). ``ValueError`` unless there are 1 .. `dumps`
        dumps and every sequence has as many entries."""
        _native_op.check_optional(input_flags, self.input_flags, "input_flags")
        if weights is not None and not self.use_weights:
            raise TypeError("weights were provided but not included in the template")
        n = len(vis)
        if not 1 <= n <= self.dumps:
            raise ValueError(f"a block has 1..{self.dumps} dumps, not {n}")
        for what, given in (("flags", flags), ("weights", weights), ("input_flags", input_flags)):
            if given is not None and len(given) != n:
                raise ValueError(f"{what} has {len(given)} entries for {n} dumps")
        fn = self._block
        fn.n_dumps = n
        inputs = {}
        for d in range(n):
            inputs[f"vis{d}"] = vis[d]
            inputs[f"flags{d}"] = flags[d]
            if self.use_weights:
                w = weights[d] if weights is not None else None
                inputs[f"weights{d}"] = w if w is not None else np.ones(np.shape(vis[d]), np.float32)
            if self.input_flags == host.BackgroundFlags.FULL:
                inputs[f"input_flags{d}"] = input_flags[d]
        if self.input_flags == host.BackgroundFlags.CHANNEL:
            if any(not np.array_equal(input_flags[0], mask) for mask in input_flags[1:]):
                raise ValueError("in CHANNEL mode a block has one mask: the entries of "
                                 "input_flags must be equal")
            inputs["input_flags"] = input_flags[0]
        _native_op.run_once(fn, self.command_queue, inputs, [])

    def finalise(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        return tuple(_native_op.run_once(self._finalise, self.command_queue, {},
                                         ["vis", "weights", "flags"]))  # fmt: skip
