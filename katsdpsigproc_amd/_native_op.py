"""What the template/operation pairs over an ahead-of-time compiled launcher have in common,
written down once. Private: the public classes live in the modules that use these
(``rfi.device``, ``rfi.ingest``, ``percentile``, ``maskedsum``, ``transpose``); DESIGN.md,
"Adding an operation", says how the pieces go together.
"""

from typing import Any, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import accel, tune
from .abc import AbstractCommandQueue, AbstractContext


class NativeTemplate:
    """Base of the templates whose kernel has one launch geometry. A subclass names its
    launcher (`KERNEL`), the reference's tuning keys it accepts without effect (`TUNING_KEYS`)
    and the class :meth:`instantiate` creates (`operation_class`), and calls :meth:`_setup`."""

    KERNEL: str
    TUNING_KEYS: Tuple[str, ...] = ()
    operation_class: type

    def _setup(self, context: AbstractContext, tuning: Optional[Mapping[str, Any]]) -> None:
        self.context = context
        self.tuning = tune.fixed_geometry(type(self).__name__, tuning, self.TUNING_KEYS)
        self.kernel = context.native_kernel(self.KERNEL)

    @classmethod
    def autotune(cls, context: AbstractContext, *args) -> Mapping[str, Any]:
        """Nothing to search, whatever the template's parameters `args`."""
        return {}

    def instantiate(self, command_queue: AbstractCommandQueue, *args, **kwargs):
        """Create an instance: the arguments of `operation_class` after the template."""
        return self.operation_class(self, command_queue, *args, **kwargs)


class AutotunedTuning:
    """``tuning`` of a template that searches: given, or autotuned on first use -- a template
    that only ever feeds the fused flagger never launches its own kernel and should not spend
    a second tuning it. `key_args` are the arguments of ``autotune`` after the context."""

    def _init_tuning(self, tuning: Optional[Mapping[str, Any]], *key_args) -> None:
        self._tuning = dict(tuning) if tuning is not None else None
        self._tuning_key = key_args

    @property
    def tuning(self) -> Mapping[str, Any]:
        if self._tuning is None:
            self._tuning = dict(self.autotune(self.context, *self._tuning_key))
        return self._tuning


class NativeOperation(accel.Operation):
    """Base of the operations on `channels` x `baselines` that launch ``template.kernel``."""

    def __init__(self, template, command_queue: AbstractCommandQueue, channels: int,
                 baselines: int, allocator: Optional[accel.AbstractAllocator] = None) -> None:  # fmt: skip
        super().__init__(command_queue, allocator)
        self.template = template
        self.kernel = template.kernel
        self.channels = channels
        self.baselines = baselines

    def _launch(self, *args) -> None:
        self.command_queue.enqueue_kernel(self.kernel, list(args))

    def layout(self, transposed: bool) -> Tuple[int, int]:
        """Shape of a channel-major (or, `transposed`, baseline-major) slot."""
        return (self.baselines, self.channels) if transposed else (self.channels, self.baselines)

    def _parameters(self, **own) -> Mapping[str, Any]:
        """`own` and the shape: what :meth:`parameters` returns."""
        return {**own, "channels": self.channels, "baselines": self.baselines}


def pointer(array: Optional[accel.DeviceArray]):
    """The launch argument for the data of `array`: None for an optional slot that is absent."""
    return array.buffer if array is not None else None


def stride(array: Optional[accel.DeviceArray], axis: int = 1) -> np.int32:
    """The launch argument for the padded length of `array` along `axis`, the row stride of
    a two-dimensional slot: 0 for an optional slot that is absent."""
    return np.int32(array.padded_shape[axis] if array is not None else 0)


def run_once(fn: accel.Operation, queue: AbstractCommandQueue, inputs: Mapping[str, Any],
             outputs: Sequence[str]) -> List[Any]:  # fmt: skip
    """The body of a host adapter: allocate the buffers of `fn`, upload `inputs` (slot name
    to array; None for an optional slot that is not there), run, download `outputs`."""
    fn.ensure_all_bound()
    for name, value in inputs.items():
        if value is not None:
            fn.buffer(name).set(queue, value)
    fn()
    return [fn.buffer(name).get(queue) for name in outputs]


def check_optional(given: Any, expected: Any, what: str) -> None:
    """``TypeError`` unless the optional input `what` is given exactly when the template has it."""
    if given is not None and not expected:
        raise TypeError(f"{what} were provided but not included in the template")
    if given is None and expected:
        raise TypeError(f"{what} were expected but not provided")
