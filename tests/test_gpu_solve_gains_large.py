"""Solving gains of up to 512 inputs on the GPU (``rfi.ingest.SolveGainsLargeTemplate``,
``ksp_solve_gains_large``): every comparison is of bit patterns, against
``rfi.host.SolveGainsLargeHost``: ``gains`` (with nothing left out but the payload of a NaN that
the host has as a NaN too), ``iterations`` and ``status``. Above 128 inputs the channels'
matrices live in a work area and a fixed grid of workgroups takes the channels in turn, so the
tests also fill the work area with other things, give workgroups a second and a third channel
with less data than the first, and look behind the bytes that are needed."""

import ctypes
import functools

import numpy as np
import pytest

from tests import inputs_solve_gains as gen
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_solve_gains import (DEFAULT, OUTPUTS, VARIANTS, assert_outputs, given_of,
                                        lonely_input)  # fmt: skip

pytestmark = pytest.mark.gpu

# The sizes at which csrc/solve_gains_large.hip changes shape: 129 is the first size with the
# matrix in the work area (one element in its fifth block of 32); a workgroup has one thread per
# input in whole wavefronts (192 up to 192 inputs, 256 up to 256, 512 at 512); 159, 160, 161 and
# 255, 256, 257 lie around a whole block, 160 and 256 are the row lengths of the planes that
# need no rounding; a thread has 16 rows in flight at a time, and the last block ends inside its
# first group of 16 at 129 (1 row), 161, 257 and 394 (10 rows) and inside its second at 159, 255
# and 511 (31 rows); 511 and 512 are the limit.
N_INPUTS = [129, 159, 160, 161, 255, 256, 257, 394, 511, 512]
SMALL_INPUTS = [1, 64, 128]  # handed to ksp_solve_gains
CHANNELS = [1, 2, 7]
WORKGROUPS = 256  # G of the kernel
f32 = np.float32


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached_case(seed, channels, n_inputs, table, data, extra):
    case = gen.make_case(seed, channels, n_inputs, table, data, extra)
    for value in case.values():
        value.setflags(write=False)  # shared between tests: nobody changes it
    return case


def want_of(case, variant, settings):
    from katsdpsigproc_amd.rfi import host

    given = given_of(case, variant)
    return host.SolveGainsLargeHost(*settings)(
        given["vis"], given["pairs"], given["weights"], given["flags"], given["initial"])


def hostile(padded_shape, dtype):
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, variant, settings, pad=0, in_place=False, work_fill=None,
               template_class=None, fn=None):  # fmt: skip
    """(gains, iterations, status) of the operation. The padding of the inputs holds NaN or
    0xFF; the outputs start out full of sentinel bytes; the work area is filled with the byte
    `work_fill` unless that is None. Afterwards every byte of padding is what it was, and so is
    every byte of the inputs. `fn`: an operation of an earlier call to run again (its work area
    then holds what that call left)."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    weights, flags, initial = variant
    channels = case["vis"].shape[0]
    n_inputs = case["pairs"].shape[0]
    given = {name: value for name, value in given_of(case, variant).items() if value is not None}
    if fn is None:
        template_class = template_class or ingest.SolveGainsLargeTemplate
        template = template_class(context, weights, flags, initial, *settings)
        fn = template.instantiate(queue, channels, case["vis"].shape[1], n_inputs)
        if pad:
            for i, name in enumerate(list(given) + ["gains"]):
                dim = fn.slots[name].dimensions[1]
                accel.Dimension(dim.size, min_padded_size=dim.size + pad + i).link(dim)
            for i, name in enumerate(["iterations", "status", "pairs"]):  # and more rows
                dim = fn.slots[name].dimensions[0]
                accel.Dimension(dim.size, min_padded_size=dim.size + pad + i).link(dim)
        if in_place:
            fn.slots["initial"].dimensions[1].link(fn.slots["gains"].dimensions[1])
        fn.ensure_all_bound()
        if in_place:
            fn.bind(gains=fn.buffer("initial"))
    assert ("work_area" in fn.slots) == (n_inputs > 128)
    if work_fill is not None and "work_area" in fn.slots:
        d = fn.buffer("work_area")
        queue.enqueue_write_buffer(d.buffer, np.full(d.padded_shape, work_fill, np.uint8))
    uploaded = {}
    for name, value in given.items():
        d = fn.buffer(name)
        assert d.padded_shape[1] >= value.shape[1] + pad
        raw = hostile(d.padded_shape, d.dtype)
        raw[: value.shape[0], : value.shape[1]] = value
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    for name in OUTPUTS:
        if not (in_place and name == "gains"):
            d = fn.buffer(name)
            queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = []
    for name in OUTPUTS:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        padding = np.ones(d.padded_shape, bool)
        padding[(slice(channels), slice(n_inputs))[: raw.ndim]] = False
        before = uploaded["initial"] if in_place and name == "gains" else sentinel_array(
            d.padded_shape, d.dtype)  # fmt: skip
        same = raw.view(np.uint8) == before.view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=-1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out.append(np.ascontiguousarray(raw[(slice(channels), slice(n_inputs))[: raw.ndim]]))
    for name, before in uploaded.items():
        if in_place and name == "initial":
            continue
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return tuple(out), fn


def compare(context, queue, case, variant, settings, what, **kwargs):
    want = want_of(case, variant, settings)
    got, _ = run_device(context, queue, case, variant, settings, **kwargs)
    assert_outputs(want, got, what)
    return want


def rotation(k, n_inputs):
    table = gen.TABLES[k % len(gen.TABLES)]
    data = gen.DATA[k % len(gen.DATA)]
    extra = (0, 37)[k % 2]
    variant = VARIANTS[k % len(VARIANTS)]
    # (8 iterations: the channel with an infinity never stops, and the host is not quick)
    settings = (8, 1e-5, min(k % 3, n_inputs - 1), 0xFF, bool(k % 2))
    return table, data, extra, variant, settings


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_sizes(n_inputs, context, command_queue):
    """Every size with 1, 2 and 7 channels; the table, the data, the width of the array (the
    full triangle, or wider with the table naming a part) and the variant rotate."""
    for i, channels in enumerate(CHANNELS):
        k = N_INPUTS.index(n_inputs) + i
        table, data, extra, variant, settings = rotation(k, n_inputs)
        case = cached_case(100 + k, channels, n_inputs, table, data, extra)
        compare(context, command_queue, case, variant, settings,
                f"{channels} channels, {n_inputs} inputs, {table}, {data}, +{extra}, {variant}")  # fmt: skip


@pytest.mark.parametrize("n_inputs", SMALL_INPUTS)
def test_small_sizes_are_solve_gains(n_inputs, context, command_queue):
    """Up to 128 inputs: no work area, the host class's results, and those of SolveGains."""
    from katsdpsigproc_amd.rfi import host, ingest

    for i, channels in enumerate(CHANNELS):
        k = SMALL_INPUTS.index(n_inputs) + i
        table, data, extra, variant, settings = rotation(k, n_inputs)
        case = cached_case(200 + k, channels, n_inputs, table, data, extra)
        want = compare(context, command_queue, case, variant, settings,
                       f"{channels} channels, {n_inputs} inputs")  # fmt: skip
        small, fn = run_device(context, command_queue, case, variant, settings,
                               template_class=ingest.SolveGainsTemplate)  # fmt: skip
        assert type(fn) is ingest.SolveGains
        assert_outputs(want, small, f"SolveGains, {channels} channels, {n_inputs} inputs")
        given = given_of(case, variant)
        old = host.SolveGainsHost(*settings)(given["vis"], given["pairs"], given["weights"],
                                             given["flags"], given["initial"])  # fmt: skip
        assert_outputs(old, want, "SolveGainsHost against SolveGainsLargeHost")


@pytest.mark.parametrize("data", gen.DATA)
@pytest.mark.parametrize("table", gen.TABLES)
def test_tables_and_data(table, data, context, command_queue):
    """Every table and data class of the inputs module, at the first size beyond LDS with a
    wider array and at a size of whole blocks."""
    for n_inputs, extra in ((129, 5), (160, 0)):
        case = cached_case(7, 3, n_inputs, table, data, extra)
        for variant in ((True, True, False), (True, True, True)):
            want = compare(context, command_queue, case, variant, DEFAULT, f"{table}, {data}")
            if data == "all_flagged":
                assert want[2][-1] & 2 and np.isnan(want[0][-1]).all()


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_variants(weights, flags, initial, context, command_queue):
    """weights / flags / initial on and off, with and without corrections, and every kind of
    reference: none, the first input, the last, and one without data."""
    n_inputs = 131
    for data in ("clean", "hostile"):
        case = cached_case(12, 2, n_inputs, "isolated", data, 3)
        lonely = lonely_input(case["pairs"])
        for corrections in (False, True):
            for reference in (-1, 0, n_inputs - 1, lonely):
                if reference in (0, n_inputs - 1) and reference == lonely:
                    continue
                settings = (12, 1e-5, reference, 0xFF, corrections)
                want = compare(context, command_queue, case, (weights, flags, initial), settings,
                               f"{data}, reference {reference}, corrections {corrections}")  # fmt: skip
                assert np.isnan(want[0][:, lonely]).all()
                if reference in (-1, lonely):
                    assert (want[2] & 4).all()
                elif data == "clean":
                    assert not (want[2] & 4).any()
                    assert (want[0][:, reference].imag == 0).all()


def staggered_case():
    """Seven clean channels whose starting gains are the truth (channel 0) or further and
    further from it, so that the channels of one launch stop at different counts."""
    case = dict(cached_case(21, 7, 140, "missing", "clean", 0))
    rs = np.random.RandomState(3)
    spread = np.exp2(rs.uniform(-1, 1, case["truth"].shape) * np.arange(7)[:, np.newaxis] / 6)
    case["initial"] = (case["truth"] * spread).astype(np.complex64)
    return case


@pytest.mark.parametrize("tol", [0.0, 1e-5, 1e-2])
@pytest.mark.parametrize("max_iterations", [1, 2, 3, 30])
def test_iterations_and_tol(max_iterations, tol, context, command_queue):
    case = staggered_case()
    settings = (max_iterations, tol, 0, 0xFF, False)
    want = compare(context, command_queue, case, (True, True, True), settings,
                   f"{max_iterations} iterations, tol {tol}")  # fmt: skip
    assert want[1].max() <= max_iterations
    if max_iterations == 1:
        assert (want[1] == 1).all() and (want[2] & 1).all()
    if max_iterations == 30 and tol == 1e-2:
        # channels of one launch stop at different counts
        assert len(set(want[1].tolist())) > 1 and not want[2].any()
        assert want[1].min() == 2 and want[1].max() < 30


# ------------------------------------------------------------ the channel loop, the work area
@functools.lru_cache(maxsize=None)
def thinning_case(channels):
    """129 inputs, every pair named; each channel has its own tenth of the samples without
    weight, and the channels a workgroup takes second and third have all but a tenth, and all
    but a thirtieth, of their samples flagged: whatever a workgroup left in its part of the work
    area from the channel before would be taken for data."""
    case = dict(gen.make_case(50, channels, 129, "complete", "clean", 0))
    rs = np.random.RandomState(51)
    shape = case["vis"].shape
    weights = case["weights"].copy()
    weights[rs.random_sample(shape) < 0.1] = 0
    flags = np.zeros(shape, np.uint8)
    chance = rs.random_sample(shape)
    flags[WORKGROUPS : 2 * WORKGROUPS][chance[WORKGROUPS : 2 * WORKGROUPS] < 0.9] = 0x04
    flags[2 * WORKGROUPS :][chance[2 * WORKGROUPS :] < 0.97] = 0x20
    case["weights"], case["flags"] = weights, flags
    for value in case.values():
        value.setflags(write=False)
    return case


@pytest.mark.parametrize("channels", [WORKGROUPS + 3, 2 * WORKGROUPS + 1])
def test_more_channels_than_workgroups(channels, context, command_queue):
    case = thinning_case(channels)
    kept = (case["flags"] == 0) & (case["weights"] > 0)
    assert kept[:WORKGROUPS].mean() > 0.85 and kept[WORKGROUPS:].mean() < 0.12
    want = compare(context, command_queue, case, (True, True, False), (6, 1e-3, 0, 0xFF, False),
                   f"{channels} channels", work_fill=0xFF)  # fmt: skip
    assert np.isfinite(want[0][:WORKGROUPS]).all()


@pytest.mark.parametrize("n_inputs", [129, 257])
def test_work_area_contents_do_not_matter(n_inputs, context, command_queue):
    """0xFF bytes (NaN), zeros, and what a call on other data left behind."""
    variant, settings = (True, True, True), (8, 1e-5, 1, 0xFF, True)
    case = cached_case(60, 3, n_inputs, "reversed", "hostile", 2)
    other = cached_case(61, 3, n_inputs, "complete", "clean", 2)
    want = want_of(case, variant, settings)
    for fill in (0xFF, 0x00):
        got, _ = run_device(context, command_queue, case, variant, settings, work_fill=fill)
        assert_outputs(want, got, f"work area of {fill:#04x}")
    got, fn = run_device(context, command_queue, other, variant, settings, work_fill=0xFF)
    assert_outputs(want_of(other, variant, settings), got, "the call before")
    got, _ = run_device(context, command_queue, case, variant, settings, fn=fn)
    assert_outputs(want, got, "after a call on other data")


# ------------------------------------------------------------------ padding, sub-views, C-ABI
@pytest.mark.parametrize("n_inputs, channels, pad", [(129, 3, 5), (160, 2, 1), (200, 1, 16),
                                                     (64, 2, 3)])  # fmt: skip
def test_padding(n_inputs, channels, pad, context, command_queue):
    """Rows padded beyond what the slots ask for, by another amount for every array (so the
    strides differ), and more rows of `pairs`, `iterations` and `status`; run_device checks
    every byte of padding and of the inputs."""
    case = cached_case(40 + pad, channels, n_inputs, "junk", "hostile", 4)
    for variant in ((True, True, True), (False, False, False), (True, False, True)):
        compare(context, command_queue, case, variant, DEFAULT, f"pad {pad}", pad=pad)
    compare(context, command_queue, case, (True, True, True), DEFAULT, f"pad {pad}, in place",
            pad=pad, in_place=True)  # fmt: skip


def raw_call(context, queue, case, variant, settings, offset, in_place=False, work_fill=0xAB,
             work_extra=64, override=None):  # fmt: skip
    """``ksp_solve_gains_large`` on sub-views `offset` elements into their allocations, each
    with an odd stride of its own. The work area is `work_extra` bytes longer than needed and
    lies between sentinels, which must survive. `override` (a dict, or a function that makes one
    from the arguments) replaces launch arguments by name, pointers as integers; the call must
    then fail, and its error message is returned in place of the outputs."""
    from katsdpsigproc_amd import _lib

    views = CompactViews(context, queue)
    given = given_of(case, variant)
    channels, baselines = case["vis"].shape
    n_inputs = case["pairs"].shape[0]
    stride_of = {"vis": (baselines + 6) | 1, "weights": (baselines + 2) | 1,
                 "flags": (baselines + 4) | 1, "pairs": (n_inputs + 2) | 1,
                 "initial": (n_inputs + 4) | 1, "gains": (n_inputs + 8) | 1}  # fmt: skip

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    d = {name: view(name, value, stride_of[name], True)
         for name, value in given.items() if value is not None and name != "initial"}  # fmt: skip
    if given["initial"] is not None:
        d["initial"] = view("initial", given["initial"], stride_of["initial"], not in_place)
    if in_place:
        d["gains"] = d["initial"]
    else:
        blank = sentinel_array((channels, n_inputs), np.complex64)
        d["gains"] = view("gains", blank, stride_of["gains"], False)
    d["iterations"] = view("iterations", sentinel_array((1, channels), np.int32), channels, False)
    d["status"] = view("status", sentinel_array((1, channels), np.uint8), channels, False)
    needed = _lib.load().ksp_solve_gains_large_work_bytes(channels, n_inputs)
    assert needed % 4 == 0 and (needed > 0) == (n_inputs > 128)
    if needed:
        content = np.full(needed, work_fill, np.uint8).view(f32)[np.newaxis]
        d["work_area"] = view("work_area", content, len(content[0]), False)
    args = {name: (d[name][1].value if name in d else None)
            for name in ("vis", "weights", "flags", "pairs", "initial", "gains", "iterations",
                         "status", "work_area")}  # fmt: skip
    args["work_bytes"] = needed + work_extra if needed else 0
    args.update(channels=channels, baselines=baselines, n_inputs=n_inputs)
    args.update({name + "_stride": (d[name][0].stride if name in d else 0) for name in stride_of})
    args.update(max_iterations=settings[0], tol2=float(f32(settings[1] * settings[1])),
                reference=settings[2], mask=settings[3], corrections=int(settings[4]))
    if override is not None:
        args.update(override(args) if callable(override) else override)
    pointers = ("vis", "weights", "flags", "pairs", "initial", "gains", "iterations", "status",
                "work_area")  # fmt: skip
    values = [ctypes.c_void_p(value) if name in pointers else value
              for name, value in args.items()]  # fmt: skip
    if override is not None:
        rc = _lib.load().ksp_solve_gains_large(context.device.index, ctypes.c_void_p(queue.stream),
                                               *values)  # fmt: skip
        assert rc != 0
        message = _lib.last_error()
    else:
        _lib.call("ksp_solve_gains_large", context.device.index, ctypes.c_void_p(queue.stream),
                  *values)  # fmt: skip
    # (read asserts that nothing around the rows changed, and nothing at all in an input)
    got = (d["gains"][0].read("gains"), d["iterations"][0].read("iterations")[0],
           d["status"][0].read("status")[0])  # fmt: skip
    for name in ("vis", "weights", "flags", "pairs", "work_area") + (
            () if in_place else ("initial",)):  # fmt: skip
        if name in d:
            d[name][0].read(name)
    if override is not None:
        # no kernel ran: the outputs and the work area are what they were
        assert not in_place and all((part.view(np.uint8) == 0xAB).all() for part in got)
        if "work_area" in d:
            assert (d["work_area"][0].read("work_area").view(np.uint8) == work_fill).all()
        return message, args
    return got, args


@pytest.mark.parametrize("channels, n_inputs, extra", [(2, 129, 0), (3, 161, 5), (1, 257, 1),
                                                       (2, 64, 1)])  # fmt: skip
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_inputs, extra, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and an odd stride of its own
    per array; the variants rotate; gains apart from initial and in place; a work area longer
    than needed between sentinels."""
    seed = 31 * offset + n_inputs
    variant = VARIANTS[seed % len(VARIANTS)]
    case = cached_case(seed, channels, n_inputs, gen.TABLES[seed % 5], "hostile", extra)
    settings = (10, 1e-5, n_inputs - 1, 0x7F, True)
    want = want_of(case, variant, settings)
    for in_place in (False, True) if variant[2] else (False,):
        got, _ = raw_call(context, command_queue, case, variant, settings, offset, in_place)
        assert_outputs(want, got, f"at {offset}, in place {in_place}")


def test_overlap_errors(context, command_queue):
    """Asserted by message; no kernel runs (raw_call finds the outputs and the work area as
    they were)."""
    case = cached_case(70, 2, 129, "complete", "clean", 0)
    channels, baselines, n_inputs = 2, case["vis"].shape[1], 129

    def message_of(override):
        message, _ = raw_call(context, command_queue, case, (True, True, True), DEFAULT, 1,
                              override=override)  # fmt: skip
        return message

    arrays = [("vis", channels, baselines, 8), ("weights", channels, baselines, 4),
              ("flags", channels, baselines, 1), ("pairs", n_inputs, n_inputs, 4),
              ("initial", channels, n_inputs, 8), ("gains", channels, n_inputs, 8),
              ("iterations", 1, channels, 4), ("status", 1, channels, 1)]  # fmt: skip
    for name, rows, cols, size in arrays:
        def starts_in_last_element(args):
            last = args[name] + ((rows - 1) * args.get(name + "_stride", 0) + cols - 1) * size
            return {"work_area": last // 4 * 4}

        def ends_in_first_element(args):
            # the first multiple of 4 from which work_bytes reach the array's first byte
            return {"work_area": ((args[name] - args["work_bytes"]) // 4 + 1) * 4}

        # (the work area is long: it may reach the allocation of an array that is checked
        # before this one, which is then the one named)
        for move in (starts_in_last_element, ends_in_first_element):
            message, args = raw_call(context, command_queue, case, (True, True, True), DEFAULT,
                                     1, override=move)  # fmt: skip
            begin, end = args["work_area"], args["work_area"] + args["work_bytes"]
            shared = [other for other, r, c, s in arrays if args[other] < end and begin < args[
                other] + ((r - 1) * args.get(other + "_stride", 0) + c) * s]  # fmt: skip
            assert name in shared
            assert f"invalid argument: work_area overlaps {shared[0]}" in message
    # vis comes first when the work area covers everything
    assert "work_area overlaps vis" in message_of(
        lambda args: {"work_area": 4096, "work_bytes": 2**62})
    assert "gains overlaps initial without being initial with the same stride" in message_of(
        lambda args: {"gains": args["initial"] + 8})
    assert "invalid argument: work_area is NULL" in message_of({"work_area": None})
    assert "invalid argument: work_area is not 4-byte aligned" in message_of(
        lambda args: {"work_area": args["work_area"] + 2})
    assert ("invalid argument: work_area is smaller than ksp_solve_gains_large_work_bytes"
            in message_of(lambda args: {"work_bytes": args["work_bytes"] - 64 - 1}))


# --------------------------------------------------------------------------------- the chain
def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    case = cached_case(11, 2, 150, "reversed", "hostile", 4)
    inputs = gen.inputs_of(case["pairs"], case["vis"].shape[1])
    for variant in ((True, True, True), (False, False, False)):
        template = ingest.SolveGainsLargeTemplate(context, *variant, max_iterations=9, mask=0x0F)
        adapter = ingest.SolveGainsLargeHostFromDevice(template, command_queue)
        given = given_of(case, variant)
        got = adapter(case["vis"], inputs, 150, given["weights"], given["flags"], given["initial"])
        assert_outputs(want_of(case, variant, (9, 1e-5, 0, 0x0F, False)), got, str(variant))


def test_in_the_chain(context, command_queue):
    """solve -> apply_gains on 8 channels of model data of 160 inputs in one sequence, the
    samples and the gains each one buffer, against SolveGainsLargeHost + ApplyGainsHost; the
    calibrated cross-correlations are the unit source (noise of 0.002 on products of gains of
    magnitude 1/2 .. 2: at most about 0.04 after calibration)."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import host, ingest

    queue = command_queue
    channels, n_inputs = 8, 160
    baselines = gen.triangle(n_inputs) + 3
    table = gen.make_table(80, "reversed", n_inputs, baselines)
    truth = gen.make_gains(81, channels, n_inputs, span=1.0)
    vis = gen.model_vis(82, truth, table, baselines, noise=0.002)
    weights = gen.make_weights(83, channels, baselines, False)
    flags = gen.make_flags(84, channels, baselines, False)
    ants = gen.inputs_of(table, baselines)
    pairs = host.SolveGainsLargeHost.pair_table(ants, n_inputs)
    solve = ingest.SolveGainsLargeTemplate(context, max_iterations=60, corrections=True).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=0x40).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    accel.Dimension(baselines, min_padded_size=baselines + 70).link(solve.slots["weights"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=200).link(apply_gains.slots["gains"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("apply_gains", apply_gains)],
        compounds={"vis": ["solve:vis", "apply_gains:vis"],
                   "weights": ["solve:weights", "apply_gains:weights"],
                   "flags": ["solve:flags", "apply_gains:flags"],
                   "gains": ["solve:gains", "apply_gains:gains"]})  # fmt: skip
    assert "solve:work_area" in seq.slots
    seq.ensure_all_bound()
    assert solve.buffer("vis") is apply_gains.buffer("vis")
    assert solve.buffer("gains") is apply_gains.buffer("gains")
    assert seq.buffer("gains").padded_shape[1] >= 200
    assert seq.buffer("solve:work_area").shape == (ingest.SolveGainsLarge.work_bytes(8, 160),)
    for name, value in (("vis", vis), ("weights", weights), ("flags", flags),
                        ("solve:pairs", pairs), ("apply_gains:inputs", ants)):  # fmt: skip
        seq.buffer(name).set(queue, value)
    seq()
    gains, iterations, status = host.SolveGainsLargeHost(max_iterations=60, corrections=True)(
        vis, pairs, weights, flags)  # fmt: skip
    cal_vis, cal_weights, cal_flags = host.ApplyGainsHost(0x40)(vis, gains, ants, weights, flags)
    for name, w in (("gains", gains), ("solve:iterations", iterations), ("solve:status", status),
                    ("apply_gains:out_vis", cal_vis), ("apply_gains:out_weights", cal_weights),
                    ("apply_gains:out_flags", cal_flags)):  # fmt: skip
        gen.assert_same(w, seq.buffer(name).get(queue), name)
    # the solution is the model's: converged, and the calibrated cross-correlations are 1
    assert not status.any()
    is_cross = ants[:, 0] != ants[:, 1]
    good = (cal_flags == 0) & is_cross[np.newaxis, :]
    assert good.mean() > 0.7 and np.abs(cal_vis[good] - 1).max() < 0.1
    turned = truth.astype(np.complex128)
    turned = turned * np.conj(turned[:, :1]) / np.abs(turned[:, :1])
    assert np.abs(1 / gains - turned).max() < 0.05
