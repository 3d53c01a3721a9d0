"""Pin everything the device operation classes do that a caller or the native library can
observe, on the fake backend: slots (shape, dtype, padding, shared dimensions, bytes), the
kernel launches with their normalised arguments, ``parameters()``, the identity of the
tuning cache entries, error texts, the host adapters' wiring and the public API.

The record is compared with ``tests/golden/device_launch_record.json``;
``python tests/test_device_launch_record.py --write`` regenerates that file. On the fake
backend a kernel computes nothing: it is the wiring that is pinned, not the results.

Two parts of the API section pin *compatibility* rather than spelling, so that a template
may inherit a forwarding ``instantiate(command_queue, *args, **kwargs)`` or an
``autotune(context, *args)`` that has nothing to search:

* a forwarding ``instantiate`` is recorded as the constructor of the ``operation_class`` it
  forwards to, without the template argument: what a caller may pass, and how;
* an ``autotune`` that is not cached takes the arguments the golden file names and answers
  ``{}``; class attributes are looked up for the (class, attribute) pairs of the golden.
"""

import ctypes
import enum
import inspect
import json
import os
import sys
import zlib

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from katsdpsigproc_amd import accel, maskedsum, percentile, transpose, tune  # noqa: E402
from katsdpsigproc_amd.rfi import device  # noqa: E402
from tests.fakes import FakeBuffer, FakeContext  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "device_launch_record.json")  # fmt: skip
MODULES = (device, percentile, maskedsum, transpose)
ATTRIBUTES = ("host_class", "transposed", "autotune_version", "SUPPORTED_WIDTHS", "TUNING_KEYS",
              "_VIS_PADS", "DEFAULT_THRESHOLD_FALLOFF")  # fmt: skip
METHODS = ("__init__", "instantiate", "autotune", "__call__", "add", "finalise")
NONE, CHANNEL, FULL = device.BackgroundFlags.NONE, device.BackgroundFlags.CHANNEL, device.BackgroundFlags.FULL


# ------------------------------------------------------------------------ normalising
def jsonable(value):
    if isinstance(value, dict):
        return {str(k): jsonable(v) for k, v in value.items()}
    if isinstance(value, (tuple, list)):
        return [jsonable(v) for v in value]
    if isinstance(value, np.generic):
        return value.item()
    if isinstance(value, np.dtype):
        return value.name
    if isinstance(value, enum.Enum):
        return value.name
    if isinstance(value, type):
        return value.__module__ + "." + value.__qualname__
    assert value is None or isinstance(value, (bool, int, float, str)), value
    return value


def buffer_names(op):
    """id of a backend buffer -> slot name, for every bound slot of `op` (a bound buffer has
    the slot's required padded shape: ``IOSlot.validate``)."""
    names = {}
    for name, slot in list(op.slots.items()) + list(op.hidden_slots.items()):
        if isinstance(slot, accel.IOSlot) and slot.buffer is not None:
            names.setdefault(id(slot.buffer.buffer), name)
    return names


def kernel_arg(arg, names):
    if arg is None:
        return None
    if isinstance(arg, FakeBuffer):
        return names.get(id(arg), f"<no slot> {arg.dtype.name}{list(arg.shape)}")
    if isinstance(arg, np.generic):
        return f"{arg.dtype.name}:{arg.item()!r}"
    if isinstance(arg, ctypes.Array):
        return f"{arg._type_.__name__}:{list(arg)!r}"
    assert isinstance(arg, (bool, int, float)), arg
    return f"{type(arg).__name__}:{arg!r}"


def launches_since(queue, first, names):
    return [[name, [kernel_arg(a, names) for a in args]] for name, args in queue.launches[first:]]


def slot_records(op):
    out = []
    for name, slot in op.slots.items():
        out.append([name, list(slot.shape), slot.dtype.name, list(slot.required_padded_shape())])
    return out


def shared_dimensions(op):
    """Groups of ``slot[axis]`` that hold one and the same Dimension object."""
    groups = {}
    for name, slot in op.slots.items():
        for axis, dim in enumerate(slot.dimensions):
            groups.setdefault(id(dim), []).append(f"{name}[{axis}]")
    return sorted(group for group in groups.values() if len(group) > 1)


class Recorder:
    """Stand-in for ``tune.autotuner_impl``: the table and key columns the cache would use."""

    def __init__(self):
        self.calls = []

    def __call__(self, test, fn, *args, **kwargs):
        cls = args[0]
        name = f"{cls.__module__}.{cls.__name__}.{fn.__name__}"
        table = name.replace(".", "_") + "__" + str(getattr(cls, "autotune_version", 0))
        self.calls.append([table, jsonable(tune._key_columns(fn, args, kwargs))])
        return test


def record_operation(make, after_bound=None):
    """Build an operation on a fresh fake context, bind, call once, and describe it."""
    queue = FakeContext().create_command_queue()
    saved, tune.autotuner_impl = tune.autotuner_impl, tune.stub_autotuner
    try:
        op = make(queue)
        rec = {
            "class": type(op).__name__,
            "slots": slot_records(op),
            "shared_dimensions": shared_dimensions(op),
            "required_bytes": op.required_bytes(),
        }
        op.ensure_all_bound()
        if after_bound is not None:
            after_bound(op)
        first = len(queue.launches)
        op()
        rec["launches"] = launches_since(queue, first, buffer_names(op))
        if not all(slot.is_bound() for slot in op.slots.values()):  # the fused flagger's options
            rec["bound"] = [name for name, slot in op.slots.items() if slot.is_bound()]
            rec["required_bytes_bound"] = op.required_bytes()
        rec["parameters"] = jsonable(op.parameters())
    finally:
        tune.autotuner_impl = saved
    return rec


def record_error(fn):
    queue = FakeContext().create_command_queue()
    saved, tune.autotuner_impl = tune.autotuner_impl, tune.stub_autotuner
    try:
        fn(queue.context, queue)
    except Exception as exc:
        return [type(exc).__name__, str(exc)]
    finally:
        tune.autotuner_impl = saved
    return None


# --------------------------------------------------------------------- configurations
#: rows of 200 are padded (to 256), rows of 50 are not; most branches show at one shape
WIDE = ((10, 200),)
BOTH = ((100, 50), (10, 200))


def flagger_template(context, use_flags=NONE, noise_t=True, thr="sum", **kw):
    bg = device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=use_flags)
    ne = (device.NoiseEstMADTDeviceTemplate(context, 10240) if noise_t
          else device.NoiseEstMADDeviceTemplate(context))  # fmt: skip
    if thr == "sum":
        th = device.ThresholdSumDeviceTemplate(context)
    else:
        th = device.ThresholdSimpleDeviceTemplate(context, thr == "simple_t")
    return device.FlaggerDeviceTemplate(bg, ne, th, **kw)


def operations():
    """(label, make(queue) -> operation, after_bound or None) for every branch."""
    out = []

    def add(label, make, after_bound=None, shapes=WIDE):
        for shape in shapes:
            out.append((f"{label} {shape[0]}x{shape[1]}",
                        lambda q, make=make, shape=shape: make(q, *shape), after_bound))  # fmt: skip

    for mode in (NONE, CHANNEL, FULL):
        for amp in (False, True):
            for tuning in (None, {"wgs": 64, "csplit": 32}):
                add(f"background {mode.name} amp={amp} tuning={tuning}",
                    lambda q, c, b, mode=mode, amp=amp, tuning=tuning:
                    device.BackgroundMedianFilterDeviceTemplate(
                        q.context, 13, amp, mode, tuning=tuning).instantiate(q, c, b),
                    shapes=BOTH if mode == FULL and not amp else WIDE)  # fmt: skip
    add("noise_mad tuning=None",
        lambda q, c, b: device.NoiseEstMADDeviceTemplate(q.context).instantiate(q, c, b))
    for method in (0, 1):
        add(f"noise_mad method={method}",
            lambda q, c, b, method=method: device.NoiseEstMADDeviceTemplate(
                q.context, tuning={"method": method}).instantiate(q, c, b),
            shapes=BOTH + ((16385, 3),))  # fmt: skip
    add("noise_madt",
        lambda q, c, b: device.NoiseEstMADTDeviceTemplate(
            q.context, 1024, tuning={"wgsx": 128}).instantiate(q, c, b), shapes=BOTH)  # fmt: skip
    for transposed in (False, True):
        add(f"threshold_simple transposed={transposed}",
            lambda q, c, b, transposed=transposed: device.ThresholdSimpleDeviceTemplate(
                q.context, transposed, flag_value=4).instantiate(q, c, b, 9.0), shapes=BOTH)  # fmt: skip
        for n_windows in (1, 8):
            add(f"threshold_sum transposed={transposed} n_windows={n_windows}",
                lambda q, c, b, transposed=transposed, n_windows=n_windows:
                device.ThresholdSumDeviceTemplate(
                    q.context, n_windows, 2, transposed=transposed).instantiate(q, c, b, 9.0, 1.5),
                shapes=BOTH if n_windows == 8 else WIDE)  # fmt: skip
        add(f"threshold_sum transposed={transposed} explicit tuning, default falloff",
            lambda q, c, b, transposed=transposed: device.ThresholdSumDeviceTemplate(
                q.context, tuning={"wgs": 256, "vt": 16},
                transposed=transposed).instantiate(q, c, b, 11.0))  # fmt: skip

    args = {"n_sigma": 11.0}
    for noise_t, thr in ((False, "simple"), (True, "simple"), (False, "simple_t"), (True, "sum")):
        add(f"flagger sequence noise_t={noise_t} threshold={thr}",
            lambda q, c, b, noise_t=noise_t, thr=thr: flagger_template(
                q.context, noise_t=noise_t, thr=thr, fused=False).instantiate(
                    q, c, b, threshold_args=args), shapes=BOTH if thr == "sum" else WIDE)  # fmt: skip
    add("flagger sequence CHANNEL input flags",
        lambda q, c, b: flagger_template(q.context, CHANNEL, fused=False).instantiate(
            q, c, b, threshold_args=args))  # fmt: skip

    fused = ((64, 200),)

    def fused_op(q, c, b, use_flags=NONE, thr="sum", threshold_args=args, **kw):
        op = flagger_template(q.context, use_flags, thr=thr, **kw).instantiate(
            q, c, b, threshold_args=threshold_args)  # fmt: skip
        assert isinstance(op, device.FusedFlaggerDevice)
        return op

    add("fused lean", fused_op, shapes=((1024, 16), (64, 200)))
    add("fused lean, vis_pad autotuned at 2048 baselines", fused_op, shapes=((64, 2048),))
    add("fused keep_deviations",
        lambda q, c, b: fused_op(q, c, b, keep_deviations=True), shapes=fused)
    add("fused deviations_t through buffer()", fused_op,
        lambda op: op.buffer("deviations_t"), shapes=fused)
    add("fused flags_t bound", fused_op,
        lambda op: op.bind(flags_t=op.slots["flags_t"].allocate(op.allocator, bind=False)),
        shapes=fused)  # fmt: skip
    add("fused vis_pad=32",
        lambda q, c, b: fused_op(q, c, b, tuning={"vis_pad": 32}), shapes=fused)
    add("fused FULL input flags, falloff 1.5",
        lambda q, c, b: fused_op(q, c, b, FULL,
                                 threshold_args={"n_sigma": 9.0, "threshold_falloff": 1.5}),
        shapes=fused)  # fmt: skip
    add("fused CHANNEL input flags", lambda q, c, b: fused_op(q, c, b, CHANNEL), shapes=fused)
    add("fused threshold_simple", lambda q, c, b: fused_op(q, c, b, thr="simple"), shapes=fused)

    for transposed in (False, True):
        for accumulate in (False, True):
            for masks in ((0xFF,), (1, 2, 4, 8, 16, 32, 64, 128)):
                add(f"flag_count transposed={transposed} accumulate={accumulate} masks={len(masks)}",
                    lambda q, c, b, transposed=transposed, accumulate=accumulate, masks=masks:
                    device.FlagCountTemplate(
                        q.context, masks, transposed, accumulate).instantiate(q, c, b),
                    shapes=BOTH if accumulate and len(masks) > 1 else WIDE)  # fmt: skip
        add(f"sir transposed={transposed}",
            lambda q, c, b, transposed=transposed: device.ScaleInvariantRankTemplate(
                q.context, 0.2, 0x0F, 16, transposed).instantiate(q, c, b), shapes=BOTH)  # fmt: skip
    for use_weights in (False, True):
        for mode in (NONE, CHANNEL, FULL):
            add(f"accumulate use_weights={use_weights} input_flags={mode.name}",
                lambda q, c, b, use_weights=use_weights, mode=mode: device.AccumulateTemplate(
                    q.context, use_weights, mode).instantiate(q, c, b),
                shapes=BOTH if use_weights and mode == FULL else WIDE)  # fmt: skip
    for factor in (1, 4):
        for clear in (False, True):
            add(f"finalise factor={factor} clear={clear}",
                lambda q, c, b, factor=factor, clear=clear: device.FinaliseTemplate(
                    q.context, factor, clear).instantiate(q, c, b),
                shapes=((100, 50), (12, 200)) if factor == 4 and clear else ((12, 200),))  # fmt: skip
    add("percentile5 column range",
        lambda q, r, c: percentile.Percentile5Template(
            q.context, 5000, tuning={"size": 64}).instantiate(q, (r, c), (10, c - 5)), shapes=BOTH)  # fmt: skip
    add("percentile5 complex, whole rows",
        lambda q, r, c: percentile.Percentile5Template(q.context, 5000, False).instantiate(q, (r, c)))
    for amplitudes in (False, True):
        add(f"maskedsum use_amplitudes={amplitudes}",
            lambda q, r, c, amplitudes=amplitudes: maskedsum.MaskedSumTemplate(
                q.context, amplitudes).instantiate(q, (r, c)), shapes=BOTH)  # fmt: skip
    add("transpose float32",
        lambda q, r, c: transpose.TransposeTemplate(q.context, np.float32, "float").instantiate(q, (r, c)),
        shapes=BOTH)
    add("transpose uint8",
        lambda q, r, c: transpose.TransposeTemplate(q.context, np.uint8, "unsigned char",
                                                    tuning={"block": 8}).instantiate(q, (r, c)))  # fmt: skip
    return out


def errors():
    """Constructor and ``instantiate`` errors that ``test_device_wiring`` does not assert."""
    sir = lambda ctx: device.ScaleInvariantRankTemplate(ctx, 0.2)  # noqa: E731
    cases = {
        "sir channels 0": lambda ctx, q: sir(ctx).instantiate(q, 0, 4),
        "sir baselines 0": lambda ctx, q: sir(ctx).instantiate(q, 4, 0),
        "sir channels 262145": lambda ctx, q: sir(ctx).instantiate(q, 262145, 4),
        "flag_count channels 0": lambda ctx, q: device.FlagCountTemplate(ctx).instantiate(q, 0, 4),
        "flag_count baselines 0": lambda ctx, q: device.FlagCountTemplate(ctx).instantiate(q, 4, 0),
        "flag_count masks=()": lambda ctx, q: device.FlagCountTemplate(ctx, masks=()),
        "flag_count adapter accumulate": lambda ctx, q: device.FlagCountHostFromDevice(
            device.FlagCountTemplate(ctx, accumulate=True), q),
        "accumulate channels 0": lambda ctx, q: device.AccumulateTemplate(ctx).instantiate(q, 0, 4),
        "finalise baselines 0": lambda ctx, q: device.FinaliseTemplate(ctx).instantiate(q, 4, 0),
        "finalise factor 3 of 100": lambda ctx, q: device.FinaliseTemplate(ctx, 3).instantiate(q, 100, 4),
        "finalise factor 0": lambda ctx, q: device.FinaliseTemplate(ctx, 0),
        "background width 4": lambda ctx, q: device.BackgroundMedianFilterDeviceTemplate(ctx, 4),
        "background use_flags=1": lambda ctx, q: device.BackgroundMedianFilterDeviceTemplate(
            ctx, 5, use_flags=1),
        "noise_madt max_channels": lambda ctx, q: device.NoiseEstMADTDeviceTemplate(ctx, 1 << 20),
        "noise_madt channels": lambda ctx, q: device.NoiseEstMADTDeviceTemplate(ctx, 64).instantiate(q, 65, 4),
        "threshold_sum n_windows 9": lambda ctx, q: device.ThresholdSumDeviceTemplate(ctx, 9),
        "fused vis_pad 3": lambda ctx, q: flagger_template(ctx, tuning={"vis_pad": 3}).instantiate(
            q, 64, 8, threshold_args={"n_sigma": 1}),
        "fused required but impossible": lambda ctx, q: flagger_template(
            ctx, noise_t=False, fused=True).instantiate(q, 16384, 8, threshold_args={"n_sigma": 1}),
        "fused n_sigma missing": lambda ctx, q: flagger_template(ctx).instantiate(q, 64, 8),
        "fused unexpected argument": lambda ctx, q: flagger_template(ctx).instantiate(
            q, 64, 8, threshold_args={"n_sigma": 1, "bogus": 2}),
        "percentile5 max_columns": lambda ctx, q: percentile.Percentile5Template(ctx, 100000),
        "percentile5 empty range": lambda ctx, q: percentile.Percentile5Template(ctx, 5000).instantiate(
            q, (10, 100), (5, 5)),
        "percentile5 range outside": lambda ctx, q: percentile.Percentile5Template(ctx, 5000).instantiate(
            q, (10, 100), (-1, 5)),
        "percentile5 range too wide": lambda ctx, q: percentile.Percentile5Template(ctx, 50).instantiate(
            q, (10, 100), (0, 51)),
        "transpose element size": lambda ctx, q: transpose.TransposeTemplate(
            ctx, np.dtype([("a", "u1", 3)]), "uchar3"),
    }  # fmt: skip
    fixed = {
        "NoiseEstMADTDeviceTemplate": lambda ctx, **kw: device.NoiseEstMADTDeviceTemplate(ctx, 4096, **kw),
        "ThresholdSimpleDeviceTemplate": lambda ctx, **kw: device.ThresholdSimpleDeviceTemplate(ctx, False, **kw),
        "FlagCountTemplate": lambda ctx, **kw: device.FlagCountTemplate(ctx, **kw),
        "ScaleInvariantRankTemplate": lambda ctx, **kw: device.ScaleInvariantRankTemplate(ctx, 0.2, **kw),
        "AccumulateTemplate": lambda ctx, **kw: device.AccumulateTemplate(ctx, **kw),
        "FinaliseTemplate": lambda ctx, **kw: device.FinaliseTemplate(ctx, **kw),
        "Percentile5Template": lambda ctx, **kw: percentile.Percentile5Template(ctx, 4096, **kw),
        "MaskedSumTemplate": lambda ctx, **kw: maskedsum.MaskedSumTemplate(ctx, **kw),
        "TransposeTemplate": lambda ctx, **kw: transpose.TransposeTemplate(ctx, np.float32, "float", **kw),
    }  # fmt: skip
    for name, make in fixed.items():
        cases[f"unknown tuning key {name}"] = (
            lambda ctx, q, make=make: make(ctx, tuning={"wavefronts": 2, "lanes": 1}))
    return {label: record_error(fn) for label, fn in cases.items()}


def tuning():
    """Which cache entry each autotuned template asks for: users' caches must keep hitting."""
    args = {"n_sigma": 11.0}
    cases = {
        "background": lambda ctx, q: device.BackgroundMedianFilterDeviceTemplate(
            ctx, 13, True, CHANNEL).instantiate(q, 10, 200)(),
        "background, tuning given": lambda ctx, q: device.BackgroundMedianFilterDeviceTemplate(
            ctx, 13, tuning={"csplit": 8}).instantiate(q, 10, 200)(),
        "noise_mad": lambda ctx, q: device.NoiseEstMADDeviceTemplate(ctx).instantiate(q, 10, 200),
        "noise_mad, tuning given": lambda ctx, q: device.NoiseEstMADDeviceTemplate(
            ctx, tuning={"method": 1}).instantiate(q, 10, 200)(),
        "threshold_sum": lambda ctx, q: device.ThresholdSumDeviceTemplate(ctx, 5).instantiate(
            q, 10, 200, 11.0)(),
        "threshold_sum, tuning given": lambda ctx, q: device.ThresholdSumDeviceTemplate(
            ctx, tuning={"vt": 8}).instantiate(q, 10, 200, 11.0)(),
        "threshold_sum transposed=False": lambda ctx, q: device.ThresholdSumDeviceTemplate(
            ctx, transposed=False).instantiate(q, 10, 200, 11.0)(),
        "flagger fused": lambda ctx, q: flagger_template(ctx, FULL).instantiate(
            q, 64, 2048, threshold_args=args)(),
        "flagger fused threshold_simple": lambda ctx, q: flagger_template(
            ctx, thr="simple").instantiate(q, 64, 200, threshold_args=args)(),
        "flagger fused, tuning given": lambda ctx, q: flagger_template(
            ctx, tuning={"vis_pad": 16}).instantiate(q, 64, 200, threshold_args=args)(),
        "flagger sequence": lambda ctx, q: flagger_template(ctx, fused=False).instantiate(
            q, 10, 200, threshold_args=args)(),
        "fused flagger alone tunes no stage": lambda ctx, q: flagger_template(ctx).instantiate(
            q, 64, 200, threshold_args=args).parameters(),
    }  # fmt: skip
    out = {}
    for label, fn in cases.items():
        queue = FakeContext().create_command_queue()
        recorder = Recorder()
        saved, tune.autotuner_impl = tune.autotuner_impl, recorder
        try:
            fn(queue.context, queue)
        finally:
            tune.autotuner_impl = saved
        out[label] = recorder.calls
    return out


# --------------------------------------------------------------------------- adapters
def record_adapter(make, call):
    """One call of a ``*HostFromDevice`` adapter: what it instantiates, launches, returns."""
    queue = FakeContext().create_command_queue()
    saved, tune.autotuner_impl = tune.autotuner_impl, tune.stub_autotuner
    made = []

    def spy(template):
        instantiate = template.instantiate

        def spied(*args, **kwargs):
            made.append(instantiate(*args, **kwargs))
            return made[-1]

        template.instantiate = spied
        return template

    try:
        adapter = make(queue.context, queue, spy)
        result = call(adapter)
        names = {}
        for op in made:
            names.update(buffer_names(op))
        results = result if isinstance(result, tuple) else (result,)
        return {
            "operations": [{"class": type(op).__name__, "slots": slot_records(op),
                            "parameters": jsonable(op.parameters())} for op in made],
            "launches": launches_since(queue, 0, names),
            "results": [[type(r).__name__, list(r.shape), r.dtype.name,
                         bool(r.flags["C_CONTIGUOUS"])] for r in results],
        }  # fmt: skip
    except Exception as exc:
        return [type(exc).__name__, str(exc)]
    finally:
        tune.autotuner_impl = saved


def adapters():
    c, b = 100, 50
    vis = np.zeros((c, b), np.complex64)
    dev = np.zeros((c, b), np.float32)
    noise = np.zeros(b, np.float32)
    flags = np.zeros((c, b), np.uint8)
    chan = np.zeros(c, np.uint8)
    bg = lambda ctx, mode: device.BackgroundMedianFilterDeviceTemplate(ctx, 13, use_flags=mode)  # noqa: E731
    flagger = lambda ctx, q, spy, mode, **kw: device.FlaggerHostFromDevice(  # noqa: E731
        spy(flagger_template(ctx, mode, **kw)), q, threshold_args={"n_sigma": 11.0})
    averager = lambda ctx, q, spy, mode=NONE, use_weights=True: device.AveragerHostFromDevice(  # noqa: E731
        spy(device.AccumulateTemplate(ctx, use_weights, mode)), spy(device.FinaliseTemplate(ctx, 4)),
        q, c, b)

    def average(adapter, **kw):
        adapter.add(vis, flags, **kw)
        return adapter.finalise()

    cases = {
        "background": (lambda ctx, q, spy: device.BackgroundHostFromDevice(spy(bg(ctx, NONE)), q),
                       lambda f: f(vis)),
        "background CHANNEL flags": (
            lambda ctx, q, spy: device.BackgroundHostFromDevice(spy(bg(ctx, CHANNEL)), q),
            lambda f: f(vis, chan)),
        "background flags not in template": (
            lambda ctx, q, spy: device.BackgroundHostFromDevice(spy(bg(ctx, NONE)), q),
            lambda f: f(vis, chan)),
        "background flags missing": (
            lambda ctx, q, spy: device.BackgroundHostFromDevice(spy(bg(ctx, FULL)), q),
            lambda f: f(vis)),
        "noise_est": (lambda ctx, q, spy: device.NoiseEstHostFromDevice(
            spy(device.NoiseEstMADDeviceTemplate(ctx)), q), lambda f: f(dev)),
        "noise_est transposed": (lambda ctx, q, spy: device.NoiseEstHostFromDevice(
            spy(device.NoiseEstMADTDeviceTemplate(ctx, 1024)), q), lambda f: f(dev)),
        "threshold simple": (lambda ctx, q, spy: device.ThresholdHostFromDevice(
            spy(device.ThresholdSimpleDeviceTemplate(ctx, False)), q, 11.0), lambda f: f(dev, noise)),
        "threshold sum, extra arguments": (lambda ctx, q, spy: device.ThresholdHostFromDevice(
            spy(device.ThresholdSumDeviceTemplate(ctx)), q, 11.0, threshold_falloff=1.5),
            lambda f: f(dev, noise)),
        "flagger sequence": (lambda ctx, q, spy: flagger(ctx, q, spy, NONE, fused=False),
                             lambda f: f(vis)),
        "flagger fused, CHANNEL flags": (lambda ctx, q, spy: flagger(ctx, q, spy, CHANNEL),
                                         lambda f: f(np.zeros((64, 24), np.complex64),
                                                     np.zeros(64, np.uint8))),
        "flagger flags not in template": (lambda ctx, q, spy: flagger(ctx, q, spy, NONE),
                                          lambda f: f(vis, chan)),
        "flagger flags missing": (lambda ctx, q, spy: flagger(ctx, q, spy, CHANNEL),
                                  lambda f: f(vis)),
        "flag_count": (lambda ctx, q, spy: device.FlagCountHostFromDevice(
            spy(device.FlagCountTemplate(ctx, (1, 2))), q), lambda f: f(flags)),
        "flag_count transposed": (lambda ctx, q, spy: device.FlagCountHostFromDevice(
            spy(device.FlagCountTemplate(ctx, transposed=True)), q), lambda f: f(flags)),
        "sir": (lambda ctx, q, spy: device.ScaleInvariantRankHostFromDevice(
            spy(device.ScaleInvariantRankTemplate(ctx, 0.2)), q), lambda f: f(flags)),
        "sir transposed": (lambda ctx, q, spy: device.ScaleInvariantRankHostFromDevice(
            spy(device.ScaleInvariantRankTemplate(ctx, 0.2, transposed=True)), q),
            lambda f: f(flags)),
        "averager": (averager, average),
        "averager weights and FULL input flags": (
            lambda ctx, q, spy: averager(ctx, q, spy, FULL),
            lambda f: average(f, weights=dev, input_flags=flags)),
        "averager input_flags not in template": (averager, lambda f: average(f, input_flags=chan)),
        "averager input_flags missing": (lambda ctx, q, spy: averager(ctx, q, spy, CHANNEL), average),
        "averager weights not in template": (
            lambda ctx, q, spy: averager(ctx, q, spy, NONE, False),
            lambda f: average(f, weights=dev)),
    }  # fmt: skip
    return {label: record_adapter(make, call) for label, (make, call) in cases.items()}


# -------------------------------------------------------------------------------- API
def parameter_list(fn, drop=()):
    """The signature without annotations (and without the parameters `drop` names)."""
    sig = inspect.signature(fn)
    params = [p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()
              if p.name not in drop]  # fmt: skip
    return str(sig.replace(parameters=params, return_annotation=inspect.Signature.empty))


def forwards(fn):
    kinds = [p.kind for p in inspect.signature(fn).parameters.values()]
    return inspect.Parameter.VAR_POSITIONAL in kinds


def api(pinned=None):
    """Public names, class attributes and signatures of the four modules. `pinned` is this
    section of the golden file (None when writing it): see the module docstring."""
    out = {}
    context = FakeContext()
    for module in MODULES:
        short = module.__name__.rsplit(".", 1)[-1]
        names = sorted(
            name for name, value in vars(module).items()
            if not name.startswith("_") and not inspect.ismodule(value)
            and getattr(value, "__module__", None) != "typing")  # fmt: skip
        entry = {"names": names, "constants": {}, "classes": {}}
        for name in names:
            value = getattr(module, name)
            if isinstance(value, (int, float, tuple)) and not isinstance(value, enum.Enum):
                entry["constants"][name] = jsonable(value)
            if not inspect.isclass(value) or value.__module__ != module.__name__:
                continue
            was = None if pinned is None else pinned[short]["classes"].get(name)
            if pinned is None:
                attributes = [a for a in dir(value) if a in ATTRIBUTES or a.startswith("MAX_")]
            else:
                attributes = list(was["attributes"]) if was else []
            cls = {"doc_crc32": zlib.crc32((value.__doc__ or "").encode()), "attributes": {}, "signatures": {}}
            for attribute in attributes:
                cls["attributes"][attribute] = jsonable(getattr(value, attribute, "<missing>"))
            for method in METHODS:
                if not any(method in vars(base) for base in value.__mro__[:-1]):
                    continue
                fn = getattr(value, method)
                if method == "instantiate" and forwards(fn):
                    params = parameter_list(value.operation_class.__init__, drop=("template",))
                elif method == "autotune" and not hasattr(fn, "test") and was and forwards(fn):
                    params = was["signatures"]["autotune"]
                    assert fn(context, *[None] * params.count(",")) == {}
                else:
                    params = parameter_list(fn)
                    if method == "autotune" and hasattr(fn, "test"):
                        params += " test=" + repr(fn.test)
                    elif method == "autotune":
                        assert fn(context, *[None] * params.count(",")) == {}
                cls["signatures"][method] = params
            entry["classes"][name] = cls
        out[short] = entry
    return out


def build_record(pinned=None):
    return {
        "operations": {label: record_operation(make, after) for label, make, after in operations()},
        "tuning": tuning(),
        "errors": errors(),
        "adapters": adapters(),
        "api": api(None if pinned is None else pinned["api"]),
    }


def dump(record) -> str:
    """One line per entry: small enough to commit, and a diff names what changed."""
    lines = []
    for section, entries in record.items():
        body = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, sort_keys=True, separators=(',', ':'))}"
                          for k, v in entries.items())  # fmt: skip
        lines.append(f" {json.dumps(section)}: {{\n{body}\n }}")
    return "{\n" + ",\n".join(lines) + "\n}\n"


def test_device_launch_record():
    with open(GOLDEN) as f:
        golden = json.load(f)
    record = json.loads(dump(build_record(golden)))
    assert list(record) == list(golden)
    for section in golden:
        assert sorted(record[section]) == sorted(golden[section]), section
        for label, expected in golden[section].items():
            assert record[section][label] == expected, f"{section}: {label}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_device_launch_record.py --write")
    text = dump(build_record())
    with open(GOLDEN, "w") as f:
        f.write(text)
    print(f"wrote {GOLDEN}: {len(text)} bytes")
