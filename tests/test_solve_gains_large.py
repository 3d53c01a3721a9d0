"""Solving gains of up to 512 inputs without a GPU: ``rfi.host.SolveGainsLargeHost`` against
the triple loop of float32 scalars of tests/test_solve_gains.py, against ``SolveGainsHost`` up
to 128 inputs and against a float64 restatement; ``pair_table`` and the argument errors at the
new limit; slot lists, the launcher chosen and every launch argument of every variant on the
fake backend; the sequence finalise -> solve -> apply_gains; the size of the work area; and the
argument checks of ``ksp_solve_gains_large``, which come before any device call."""

import ctypes
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_solve_gains as gen
from tests.fakes import FakeContext
from tests.inputs_solve_gains import assert_same
from tests.test_solve_gains import (ARRAYS, STRIDES, VARIANTS, arguments, expected_slots,
                                    solve_float64, triple_loop)  # fmt: skip

f32 = np.float32
LARGE, SMALL = host.SolveGainsLargeHost, host.SolveGainsHost


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def assert_results(want, got, what=""):
    assert_same(want[0], got[0], f"gains {what}")
    for name, w, g in zip(("iterations", "status"), want[1:], got[1:]):
        assert w.dtype == g.dtype and (w == g).all(), (name, what, w, g)


# ------------------------------------------------------------------------------ the host class
@pytest.mark.parametrize("n_inputs, channels, table, data, variant, settings", [
    (129, 2, "junk", "hostile", (True, True, True), (3, 1e-5, 128, 0xFF, True)),
    (160, 1, "reversed", "clean", (True, False, False), (4, 1e-2, 0, 0xFF, False)),
    (257, 1, "isolated", "hostile", (False, True, True), (2, 0.0, -1, 0x0F, False)),
])  # fmt: skip
def test_host_against_triple_loop(n_inputs, channels, table, data, variant, settings):
    case = gen.make_case(n_inputs, channels, n_inputs, table, data, extra=2)
    before = {name: value.copy() for name, value in case.items()}
    args = arguments(case, *variant)
    got = LARGE(*settings)(*args)
    assert_results(triple_loop(*args, *settings), got)
    assert all(g.flags.c_contiguous for g in got)
    for name, value in case.items():  # the inputs are never modified
        assert_same(before[name].view(np.uint8), value.view(np.uint8), name)


@pytest.mark.parametrize("data", gen.DATA)
@pytest.mark.parametrize("n_inputs", [1, 33, 64, 128])
def test_equals_solve_gains_host_up_to_128(n_inputs, data):
    for i, variant in enumerate([(True, True, True), (False, True, False)]):
        table = gen.TABLES[(n_inputs + i) % len(gen.TABLES)]
        case = gen.make_case(3 + i, 3, n_inputs, table, data, extra=i)
        settings = (12, 1e-5, n_inputs - 1, 0xFF, bool(i))
        args = arguments(case, *variant)
        assert_results(SMALL(*settings)(*args), LARGE(*settings)(*args), f"{table}, {data}")


def test_constants_and_pair_table():
    assert LARGE.MAX_INPUTS == 512 and LARGE.BLOCK == 32 and issubclass(LARGE, SMALL)
    assert SMALL.MAX_INPUTS == 128 and SMALL.BLOCK == 32
    assert (LARGE.MAX_ITERATIONS, LARGE.NOT_CONVERGED, LARGE.NO_DATA, LARGE.NOT_REFERENCED) == (
        1000, 1, 2, 4)  # fmt: skip
    table = gen.make_table(1, "reversed", 512, gen.triangle(512) + 9)
    inputs = gen.inputs_of(table, gen.triangle(512) + 9)
    back = LARGE.pair_table(inputs, 512)
    assert back.shape == (512, 512) and back.dtype == np.int32
    upper = np.triu_indices(512, 1)
    assert (back[upper] == table[upper]).all() and (back[upper] != 0).mean() > 0.85
    assert not back[np.tril_indices(512)].any()
    for bad in (0, 513, -1):
        with pytest.raises(ValueError, match=r"n_inputs must be 1\.\.512"):
            LARGE.pair_table(inputs, bad)
    with pytest.raises(ValueError, match=r"n_inputs must be 1\.\.128"):
        SMALL.pair_table(inputs, 129)
    with pytest.raises(TypeError, match="n_inputs"):
        LARGE.pair_table(inputs, 512.0)
    with pytest.raises(ValueError, match="twice"):
        LARGE.pair_table(np.array([[0, 300], [300, 0]], np.int32), 512)


def test_host_errors():
    for bad in (-2, 512, 1000):
        with pytest.raises(ValueError, match=r"reference must be -1\.\.511"):
            LARGE(reference=bad)
    assert LARGE(reference=511).reference == 511
    with pytest.raises(ValueError, match=r"reference must be -1\.\.127"):
        SMALL(reference=128)
    for bad in (0, 1001):
        with pytest.raises(ValueError, match=r"max_iterations must be 1\.\.1000"):
            LARGE(max_iterations=bad)
    vis = np.ones((2, 3), np.complex64)
    for n in (0, 513):
        with pytest.raises(ValueError, match=r"pairs.*n_inputs 1\.\.512"):
            LARGE()(vis, np.zeros((n, n), np.int32))
    with pytest.raises(ValueError, match=r"pairs.*n_inputs 1\.\.128"):
        SMALL()(vis, np.zeros((129, 129), np.int32))
    gains, iterations, status = LARGE()(vis, np.zeros((512, 512), np.int32))
    assert gains.shape == (2, 512) and np.isnan(gains).all() and (status == 2 | 4).all()
    assert (iterations == 2).all()  # (nothing moves: 0 <= 0 after the first even iteration)
    with pytest.raises(ValueError, match="reference must be -1 or 0..n_inputs-1 = 199, not 200"):
        LARGE(reference=200)(vis, np.zeros((200, 200), np.int32))
    LARGE(reference=199)(vis, np.zeros((200, 200), np.int32))
    with pytest.raises(ValueError, match="initial"):
        LARGE()(vis, np.zeros((200, 200), np.int32), initial=np.ones((2, 199), np.complex64))


# ------------------------------------------------------------------------------ accuracy
#: the largest relative difference measured on the cases below
MEASURED_ACCURACY = 2.58e-7


@pytest.mark.parametrize("max_iterations", [10, 30])
def test_accuracy_against_float64(max_iterations):
    """As tests/test_solve_gains.py does up to 64 inputs: tol=0 and a fixed count, so both
    precisions run the same iterations; gains of magnitude 2^U(-3, 3), about 10 % of the pairs
    missing, 1 % noise. Relative difference: the largest |g32 - g64| of a channel over its
    largest |g64|."""
    worst = 0.0
    for seed in gen.ACCURACY_SEEDS[:2]:
        for n in (160, 394, 512):
            case = gen.make_case(seed, 1, n, "missing", "clean", extra=1)
            g32 = LARGE(max_iterations, tol=0.0)(case["vis"], case["pairs"], case["weights"])[0]
            g64 = solve_float64(case["vis"], case["pairs"], case["weights"], max_iterations)
            assert np.isfinite(g32).all()
            relative = np.abs(g32 - g64).max(axis=1) / np.abs(g64).max(axis=1)
            worst = max(worst, float(relative.max()))
    print(f"largest relative difference at {max_iterations} iterations: {worst:.3e}")
    assert worst <= 2 * MEASURED_ACCURACY


# ------------------------------------------------------------- template, operation, adapter
def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.SolveGainsLargeTemplate(context, tuning={"wgs": 256})
    assert ingest.SolveGainsLargeTemplate(context, tuning={}).tuning == {}
    assert ingest.SolveGainsLargeTemplate.autotune(context) == {}
    assert ingest.SolveGainsLargeTemplate.host_class is LARGE
    assert ingest.SolveGainsLargeTemplate.KERNEL == "ksp_solve_gains_large"
    assert ingest.SolveGainsLargeTemplate.operation_class is ingest.SolveGainsLarge
    assert ingest.SolveGainsTemplate.operation_class is ingest.SolveGains
    for keyword, bad, error in [
            ("max_iterations", 0, ValueError), ("max_iterations", 1001, ValueError),
            ("max_iterations", 2.0, TypeError), ("tol", -1.0, ValueError),
            ("reference", -2, ValueError), ("reference", 512, ValueError),
            ("reference", 1.5, TypeError), ("mask", 256, ValueError),
            ("mask", 0.5, TypeError)]:  # fmt: skip
        with pytest.raises(error, match=keyword):
            ingest.SolveGainsLargeTemplate(context, **{keyword: bad})
    with pytest.raises(ValueError, match=r"reference must be -1\.\.127"):
        ingest.SolveGainsTemplate(context, reference=128)
    template = ingest.SolveGainsLargeTemplate(context)
    assert template.kernel.name == "ksp_solve_gains_large"
    assert template.small_kernel.name == "ksp_solve_gains"
    assert (template.weights, template.flags, template.initial) == (True, True, False)
    assert (template.max_iterations, template.tol, template.reference, template.mask,
            template.corrections) == (30, 1e-5, 0, 0xFF, False)  # fmt: skip
    assert template.tol2 == f32(1e-10)
    for args in [(0, 4, 200), (4, 0, 200), (4, 4, 0), (4, 4, -1), (4, 4, 513)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    with pytest.raises(ValueError, match=r"n_inputs must be 1\.\.512"):
        template.instantiate(queue, 4, 4, 513)
    with pytest.raises(ValueError, match="reference"):
        ingest.SolveGainsLargeTemplate(context, reference=300).instantiate(queue, 4, 4, 300)
    fn = ingest.SolveGainsLargeTemplate(context, reference=299).instantiate(queue, 4, 4, 300)
    assert type(fn) is ingest.SolveGainsLarge
    assert type(template.instantiate(queue, 4, 5, 512)) is ingest.SolveGainsLarge
    assert template.instantiate(queue, 2, 1, 130).parameters() == {
        "weights": True, "flags": True, "initial": False, "max_iterations": 30, "tol": 1e-5,
        "reference": 0, "mask": 255, "corrections": False, "n_inputs": 130, "channels": 2,
        "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 2, 130, "reversed", "clean", extra=2)
    baselines = case["vis"].shape[1]
    inputs = gen.inputs_of(case["pairs"], baselines)
    for weights, flags, initial in VARIANTS:
        template = ingest.SolveGainsLargeTemplate(context, weights=weights, flags=flags,
                                                  initial=initial)  # fmt: skip
        adapter = ingest.SolveGainsLargeHostFromDevice(template, queue)
        given = {"weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None,
                 "initial": case["initial"] if initial else None}  # fmt: skip
        del queue.launches[:]
        gains, iterations, status = adapter(case["vis"], inputs, 130, **given)
        assert (gains.shape, gains.dtype) == ((2, 130), np.complex64)
        assert (iterations.shape, iterations.dtype) == ((2,), np.int32)
        assert (status.shape, status.dtype) == ((2,), np.uint8)
        assert [name for name, _ in queue.launches] == ["ksp_solve_gains_large"]
        args = queue.launches[0][1]
        assert [int(a) for a in args[10:13]] == [2, baselines, 130]
        assert (args[3].array[:130, :130] == LARGE.pair_table(inputs, 130)).all()
        for name in ("weights", "flags", "initial"):
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(case["vis"], inputs, 130, **wrong)
    adapter = ingest.SolveGainsLargeHostFromDevice(
        ingest.SolveGainsLargeTemplate(context, False, False), queue)  # fmt: skip
    with pytest.raises(ValueError, match="inputs"):
        adapter(case["vis"], inputs[:-1], 130)
    with pytest.raises(ValueError, match=r"n_inputs must be 1\.\.512"):
        adapter(case["vis"], inputs, 513)
    with pytest.raises(ValueError, match="twice"):
        adapter(case["vis"], np.zeros((baselines, 2), np.int32) + [0, 1], 130)
    # up to 128 inputs the adapter reaches the launcher of SolveGains
    small = gen.make_case(1, 2, 5, "reversed", "clean")
    del queue.launches[:]
    adapter(small["vis"], gen.inputs_of(small["pairs"], 10), 5)
    assert [name for name, _ in queue.launches] == ["ksp_solve_gains"]


# ------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
@pytest.mark.parametrize("n_inputs", [128, 129])
def test_slots(n_inputs, weights, flags, initial, context, queue):
    template = ingest.SolveGainsLargeTemplate(context, weights=weights, flags=flags,
                                              initial=initial)  # fmt: skip
    fn = template.instantiate(queue, 300, 200, n_inputs)
    large = n_inputs > 128
    assert list(fn.slots) == expected_slots(weights, flags, initial) + ["work_area"] * large
    n, work_bytes = n_inputs, 256 * 3 * 129 * 160 * 4
    shapes = {"vis": ((300, 200), np.complex64), "weights": ((300, 200), np.float32),
              "flags": ((300, 200), np.uint8), "pairs": ((n, n), np.int32),
              "initial": ((300, n), np.complex64), "gains": ((300, n), np.complex64),
              "iterations": ((300,), np.int32), "status": ((300,), np.uint8),
              "work_area": ((work_bytes,), np.uint8)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots) - 2 - large
    if large:
        assert fn.slots["work_area"].dimensions[0].exact
    assert fn.parameters()["n_inputs"] == n_inputs and fn.parameters()["initial"] == initial


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
@pytest.mark.parametrize("n_inputs", [128, 129])
def test_launch_arguments(n_inputs, weights, flags, initial, context, queue):
    """At 128 inputs the launcher, and every argument, are those of SolveGains; at 129 the work
    area and its size stand behind the arrays."""
    large = n_inputs > 128
    settings = dict(weights=weights, flags=flags, initial=initial, max_iterations=17, tol=1e-3,
                    reference=19, mask=0x41, corrections=True)  # fmt: skip
    fn = ingest.SolveGainsLargeTemplate(context, **settings).instantiate(queue, 300, 200, n_inputs)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["vis"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=170).link(fn.slots["gains"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == [
        "ksp_solve_gains_large" if large else "ksp_solve_gains"]  # fmt: skip
    args = queue.launches[0][1]
    assert len(args) == 24 if large else 22

    def buf(name, present=True):
        return fn.buffer(name).buffer if present else None

    pointers = [buf("vis"), buf("weights", weights), buf("flags", flags), buf("pairs"),
                buf("initial", initial), buf("gains"), buf("iterations"), buf("status")]  # fmt: skip
    for got, want in zip(args[:8], pointers):
        assert got is want
    if large:
        work_bytes = 256 * 3 * 129 * 160 * 4
        assert args[8] is buf("work_area") and args[8] not in pointers
        assert isinstance(args[9], np.uint64) and int(args[9]) == work_bytes
        assert fn.buffer("work_area").padded_shape == (work_bytes,)
        rest = args[10:]
    else:
        rest = args[8:]
        old = ingest.SolveGainsTemplate(context, **settings).instantiate(queue, 300, 200, n_inputs)
        accel.Dimension(200, min_padded_size=500).link(old.slots["vis"].dimensions[1])
        accel.Dimension(n_inputs, min_padded_size=170).link(old.slots["gains"].dimensions[1])
        old()
        assert queue.launches[1][0] == "ksp_solve_gains"
        assert [(type(a), a) for a in queue.launches[1][1][8:]] == [(type(a), a) for a in rest]
    assert all(isinstance(a, np.int32) for a in rest[:10] + rest[11:])
    assert [int(a) for a in rest[:3]] == [300, 200, n_inputs]

    def stride(name, present=True):
        return fn.buffer(name).padded_shape[1] if present else 0

    strides = [stride("vis"), stride("weights", weights), stride("flags", flags), stride("pairs"),
               stride("initial", initial), stride("gains")]  # fmt: skip
    assert [int(a) for a in rest[3:9]] == strides
    # 500 and 170 rounded up to whole 128-byte rows; the others as their own slots ask
    assert strides == [512, 224 if weights else 0, 256 if flags else 0,
                       128 if n_inputs == 128 else 160, (128 if n_inputs == 128 else 144) if
                       initial else 0, 176]  # fmt: skip
    assert int(rest[9]) == 17
    assert isinstance(rest[10], np.float32) and rest[10] == f32(1e-3 * 1e-3)
    assert [int(a) for a in rest[11:]] == [19, 0x41, 1]


def test_refining_in_place(context, queue):
    fn = ingest.SolveGainsLargeTemplate(context, initial=True).instantiate(queue, 16, 40, 200)
    fn.slots["initial"].dimensions[1].link(fn.slots["gains"].dimensions[1])
    fn.ensure_all_bound()
    fn.bind(gains=fn.buffer("initial"))
    fn()
    args = queue.launches[0][1]
    assert args[4] is args[5] is fn.buffer("initial").buffer
    assert int(args[17]) == int(args[18]) == fn.buffer("gains").padded_shape[1]


def test_between_finalise_and_apply_gains(context, queue):
    """finalise -> solve -> apply_gains at 160 inputs: the averaged arrays are the samples of
    both, each one buffer with one padded size, the solver's `gains` are the `gains` that are
    applied, and the work area is a slot of the sequence."""
    channels, baselines, cf, n_inputs = 1024, 200, 8, 160
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveGainsLargeTemplate(context, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=200).link(apply_gains.slots["gains"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("solve", solve), ("apply_gains", apply_gains)],
        compounds={"vis": ["finalise:vis", "solve:vis", "apply_gains:vis"],
                   "weights": ["finalise:weights", "solve:weights", "apply_gains:weights"],
                   "flags": ["finalise:flags", "solve:flags", "apply_gains:flags"],
                   "gains": ["solve:gains", "apply_gains:gains"]})  # fmt: skip
    assert {"vis", "weights", "flags", "gains", "solve:pairs", "solve:iterations", "solve:status",
            "solve:work_area", "apply_gains:inputs", "apply_gains:out_vis"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_finalise", "ksp_solve_gains_large", "ksp_apply_gains"]  # fmt: skip
    final_args, solve_args, apply_args = (launch[1] for launch in queue.launches)
    assert final_args[3] is solve_args[0] is apply_args[0] is seq.buffer("vis").buffer
    assert final_args[4] is solve_args[1] is apply_args[1] is seq.buffer("weights").buffer
    assert final_args[5] is solve_args[2] is apply_args[2] is seq.buffer("flags").buffer
    assert solve_args[5] is apply_args[3] is seq.buffer("gains").buffer
    assert solve_args[8] is seq.buffer("solve:work_area").buffer
    assert int(solve_args[9]) == ingest.SolveGainsLarge.work_bytes(rows, n_inputs)
    assert int(final_args[14]) == int(solve_args[14]) == int(apply_args[12]) == 320
    assert int(final_args[13]) == int(solve_args[13]) == int(apply_args[11])
    assert int(final_args[15]) == int(solve_args[15]) == int(apply_args[13])
    assert int(solve_args[18]) == int(apply_args[14]) == seq.buffer("gains").padded_shape[1] == 208
    assert [int(a) for a in solve_args[10:13]] == [rows, baselines, n_inputs]
    assert int(solve_args[23]) == 1


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_work_bytes(lib):
    work_bytes = ingest.SolveGainsLarge.work_bytes
    assert ingest.SolveGainsLarge.WORKGROUPS == 256
    for args in [(1, 129), (2, 129), (255, 160), (256, 160), (257, 161), (4096, 394), (7, 511),
                 (1, 512), (1000000, 512), (2**31 - 1, 512)]:  # fmt: skip
        assert lib.ksp_solve_gains_large_work_bytes(*args) == work_bytes(*args) > 0, args
    for args in [(0, 200), (-1, 200), (4, 0), (4, -1), (4, 1), (4, 128), (4, 513)]:
        assert lib.ksp_solve_gains_large_work_bytes(*args) == work_bytes(*args) == 0, args
    assert work_bytes(1, 129) == 3 * 129 * 160 * 4
    assert work_bytes(300, 160) == 256 * 3 * 160 * 160 * 4
    assert work_bytes(1, 512) == 3 * 2**20
    # the formula: min(G, channels) slots, whatever the number of channels
    assert work_bytes(1000000, 512) == work_bytes(256, 512) == 768 * 2**20 <= 2**30


LARGE_ARRAYS = ARRAYS + ["work_area"]


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Nine arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(LARGE_ARRAYS)}

    def call(channels=4, baselines=8, n_inputs=130, max_iterations=30, tol2=1e-10, reference=0,
             mask=255, corrections=0, work_bytes=None, **changed):  # fmt: skip
        a = dict(p, vis_stride=8, weights_stride=8, flags_stride=8, pairs_stride=130,
                 initial_stride=130, gains_stride=130)  # fmt: skip
        a.update(changed)
        if work_bytes is None:
            work_bytes = lib.ksp_solve_gains_large_work_bytes(channels, n_inputs)
        rc = lib.ksp_solve_gains_large(
            0, None, *(a[name] for name in LARGE_ARRAYS), work_bytes, channels, baselines,
            n_inputs, *(a[name + "_stride"] for name in STRIDES), max_iterations, tol2,
            reference, mask, corrections)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    # ---- the messages of ksp_solve_gains, character for character, with the new limit
    for name in ("vis", "pairs", "gains", "iterations", "status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -1, 513):
        assert "invalid argument: n_inputs must be 1..512" in call(n_inputs=bad)
    for bad in (0, -1, 1001):
        assert "invalid argument: max_iterations must be 1..1000" in call(max_iterations=bad)
    for bad in (-1e-20, float("nan"), -float("inf")):
        assert "invalid argument: tol2 must be at least 0" in call(tol2=bad)
    for bad in (-2, 130, 512):
        assert "invalid argument: reference must be -1..n_inputs-1" in call(reference=bad)
    for bad in (-1, 256):
        assert "invalid argument: mask must be 0..255" in call(mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for name in ("vis", "weights", "flags"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})
    for name in ("pairs", "initial", "gains"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 129})
    assert "gains_stride is smaller" in call(n_inputs=512, pairs_stride=512, initial_stride=512,
                                             gains_stride=511)  # fmt: skip
    # up to 128 inputs the same checks run here, before the call is handed on
    assert "invalid argument: pairs_stride is smaller than n_inputs" in call(
        n_inputs=128, pairs_stride=127, work_area=None, work_bytes=0)
    assert "invalid argument: reference must be -1..n_inputs-1" in call(
        n_inputs=64, reference=64, work_area=None, work_bytes=0)

    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    overlap = "gains overlaps initial without being initial with the same stride"
    extent = (3 * 130 + 130) * 8  # the bytes from the first element to the last
    assert overlap in call(gains=at("initial", 8))
    assert overlap in call(gains=at("initial", extent - 1))
    assert overlap in call(gains=at("initial", -(extent - 1)))
    assert overlap in call(gains=p["initial"], gains_stride=131)  # same pointer, other stride

    # ---- the new messages
    needed = lib.ksp_solve_gains_large_work_bytes(4, 130)
    assert needed == 4 * 3 * 130 * 160 * 4
    null = "invalid argument: work_area is NULL"
    aligned = "invalid argument: work_area is not 4-byte aligned"
    small = "invalid argument: work_area is smaller than ksp_solve_gains_large_work_bytes"
    assert null in call(work_area=None)
    for offset in (1, 2, 3, 5):
        assert aligned in call(work_area=at("work_area", offset))
    for bad in (0, 1, needed - 1):
        assert small in call(work_bytes=bad)
    # each array's first and last byte of data, with the work area ending or starting there
    extents = {"vis": (3 * 8 + 8) * 8, "weights": (3 * 8 + 8) * 4, "flags": 3 * 8 + 8,
               "pairs": (129 * 130 + 130) * 4, "initial": extent, "gains": extent,
               "iterations": 4 * 4, "status": 4}  # fmt: skip
    for name in ARRAYS:
        message = f"invalid argument: work_area overlaps {name}"
        assert message in call(work_area=at(name, extents[name] - 4))
        assert message in call(work_area=at(name, -needed + 4))
        assert message in call(work_area=at(name, -needed - 60), work_bytes=needed + 64)
        # (an area that only touches the array passes this check and fails the next)
        assert "corrections must" in call(work_area=at(name, -needed), corrections=2)
    absent = dict(weights=None, flags=None, initial=None, weights_stride=0, flags_stride=0,
                  initial_stride=0)  # fmt: skip
    assert "work_area overlaps pairs" in call(work_area=at("pairs", 0), **absent)
    assert "work_area overlaps vis" in call(work_area=ctypes.c_void_p(4096), work_bytes=2**62)

    # ---- the order: everything of ksp_solve_gains first, in its order, then the work area:
    # NULL, alignment, size, overlap
    strides = {name + "_stride": -1 for name in STRIDES}
    wrong = dict(channels=0, baselines=0, n_inputs=0, max_iterations=0, tol2=-1.0, reference=-2,
                 mask=-1, corrections=2)  # fmt: skip
    nothing = dict.fromkeys(LARGE_ARRAYS)
    assert "invalid argument: vis is NULL" in call(**wrong, **nothing, **strides, work_bytes=0)
    assert "invalid argument: iterations is NULL" in call(
        **wrong, iterations=None, status=None, work_area=None, work_bytes=0, **strides)
    order = ["channels must", "baselines must", "n_inputs must", "max_iterations must",
             "tol2 must", "reference must", "mask must", "corrections must"]  # fmt: skip
    keys = list(wrong)
    for i, message in enumerate(order):
        assert message in call(**{key: wrong[key] for key in keys[i:]}, **strides,
                               work_area=None, work_bytes=0)  # fmt: skip
    assert "vis_stride is smaller than baselines" in call(**strides, work_area=None, work_bytes=0)
    bad_work = dict(work_area=None, work_bytes=0)
    assert "gains_stride is smaller" in call(gains_stride=2, **bad_work)
    assert overlap in call(gains=at("initial", 8), **bad_work)
    assert null in call(**bad_work)
    assert aligned in call(work_area=at("vis", 1), work_bytes=0)
    assert small in call(work_area=at("vis", 0), work_bytes=0)
    assert "work_area overlaps vis" in call(work_area=at("vis", 0))


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def names_of(function):
        declaration = re.search(r"\b%s\((.*?)\);" % function, text, re.S)
        assert declaration is not None
        parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
        return parameters, [parameter.replace("*", " ").split()[-1] for parameter in parameters]

    parameters, names = names_of("int ksp_solve_gains_large")
    argtypes = _lib.SIGNATURES["ksp_solve_gains_large"]
    assert len(parameters) == len(argtypes) == 26
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert (parameter.split()[0] == "float") == (argtype is ctypes.c_float), parameter
        assert (parameter.split()[0] == "size_t") == (argtype is ctypes.c_size_t), parameter
    # the arguments of ksp_solve_gains, with the work area and its size behind the arrays
    old = names_of("int ksp_solve_gains")[1]
    assert names == old[:10] + ["work_area", "work_bytes"] + old[10:]
    assert names_of("size_t ksp_solve_gains_large_work_bytes")[1] == ["channels", "n_inputs"]
    assert _lib._OTHER["ksp_solve_gains_large_work_bytes"] == (
        [ctypes.c_int, ctypes.c_int], ctypes.c_size_t)  # fmt: skip
    for name in ("ksp_solve_gains_large", "ksp_solve_gains_large_work_bytes", "ksp_solve_gains"):
        assert hasattr(lib, name) and name in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("SolveGainsLargeTemplate", "SolveGainsLarge", "SolveGainsLargeHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "SolveGainsLargeHost")
