"""Solving gains on the GPU (``rfi.ingest.SolveGainsTemplate``, ``ksp_solve_gains``): every
comparison is of bit patterns, against ``rfi.host.SolveGainsHost``: ``gains`` (with nothing
left out but the payload of a NaN that the host has as a NaN too), ``iterations`` and
``status``."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import inputs_solve_gains as gen
from tests.inputs_solve_gains import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import LOST, N_AUTO

pytestmark = pytest.mark.gpu

# The sizes at which csrc/solve_gains.hip changes shape: a sum runs in blocks of 32 inputs, so
# 32, 64 and 96 are the last sizes with 1, 2 and 3 blocks; the workgroup has n * blocks threads
# rounded up to whole wavefronts (64 for up to 32 inputs, 512 for 128); 1 input has an empty
# triangle, and 128 is the limit.
N_INPUTS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 127, 128]
CHANNELS = [1, 2, 7]
VARIANTS = list(itertools.product([True, False], repeat=3))  # weights, flags, initial
OUTPUTS = ("gains", "iterations", "status")
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


def given_of(case, variant):
    weights, flags, initial = variant
    return {"vis": case["vis"], "pairs": case["pairs"],
            "weights": case["weights"] if weights else None,
            "flags": case["flags"] if flags else None,
            "initial": case["initial"] if initial else None}  # fmt: skip


def want_of(case, variant, settings):
    from katsdpsigproc_amd.rfi import host

    given = given_of(case, variant)
    return host.SolveGainsHost(*settings)(
        given["vis"], given["pairs"], given["weights"], given["flags"], given["initial"])


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF (a `pairs` entry of -1, which
    would name baseline 0, and a flag byte that is all set)."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, variant, settings, pad=0, in_place=False):
    """(gains, iterations, status) of the operation. The padding of the inputs holds NaN or
    0xFF; the outputs start out full of sentinel bytes. Afterwards every byte of padding is what
    it was, and so is every byte of the inputs."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    weights, flags, initial = variant
    channels = case["vis"].shape[0]
    n_inputs = case["pairs"].shape[0]
    template = ingest.SolveGainsTemplate(context, weights, flags, initial, *settings)
    fn = template.instantiate(queue, channels, case["vis"].shape[1], n_inputs)
    given = {name: value for name, value in given_of(case, variant).items() if value is not None}
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
    return tuple(out)


def assert_outputs(want, got, what):
    assert_same(want[0], got[0], f"gains {what}")
    for name, w, g in zip(OUTPUTS[1:], want[1:], got[1:]):
        assert w.dtype == g.dtype and w.shape == g.shape, name
        assert (w == g).all(), f"{name} {what}: want {w}, got {g}"


def compare(context, queue, case, variant, settings, what, pad=0, in_place=False):
    want = want_of(case, variant, settings)
    got = run_device(context, queue, case, variant, settings, pad, in_place)
    assert_outputs(want, got, what)
    return want


DEFAULT = (30, 1e-5, 0, 0xFF, False)


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_sizes(n_inputs, context, command_queue):
    """Every size with 1, 2 and 7 channels; the table, the data, the width of the array (the
    full triangle, or wider with the table naming a part) and the variant rotate."""
    for i, channels in enumerate(CHANNELS):
        k = N_INPUTS.index(n_inputs) + i
        table = gen.TABLES[k % len(gen.TABLES)]
        data = gen.DATA[k % len(gen.DATA)]
        extra = (0, 37)[k % 2]
        variant = VARIANTS[k % len(VARIANTS)]
        case = cached_case(100 + k, channels, n_inputs, table, data, extra)
        settings = (30, 1e-5, min(k % 3, n_inputs - 1), 0xFF, bool(k % 2))
        compare(context, command_queue, case, variant, settings,
                f"{channels} channels, {n_inputs} inputs, {table}, {data}, +{extra}, {variant}")  # fmt: skip


@pytest.mark.parametrize("data", gen.DATA)
@pytest.mark.parametrize("table", gen.TABLES)
def test_tables_and_data(table, data, context, command_queue):
    """Every table and data class of the inputs module, at a size of two blocks and one that
    fills a wavefront exactly."""
    for n_inputs, extra in ((33, 0), (8, 5)):
        case = cached_case(7, 3, n_inputs, table, data, extra)
        for variant in ((True, True, False), (True, True, True)):
            want = compare(context, command_queue, case, variant, DEFAULT, f"{table}, {data}")
            if data == "all_flagged":
                assert want[2][-1] & 2 and np.isnan(want[0][-1]).all()


def lonely_input(pairs):
    p, q = np.triu_indices(pairs.shape[0], 1)
    used = np.zeros(pairs.shape[0], bool)
    valid = pairs[p, q] != 0
    used[p[valid]] = used[q[valid]] = True
    return int(np.flatnonzero(~used)[0])


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_variants(weights, flags, initial, context, command_queue):
    """weights / flags / initial on and off, with and without corrections, and every kind of
    reference: none, the first input, the last, and one without data."""
    n_inputs = 34
    for data in ("clean", "hostile"):
        case = cached_case(12, 2, n_inputs, "isolated", data, 3)
        lonely = lonely_input(case["pairs"])
        for corrections in (False, True):
            for reference in (-1, 0, n_inputs - 1, lonely):
                if reference in (0, n_inputs - 1) and reference == lonely:
                    continue
                settings = (30, 1e-5, reference, 0xFF, corrections)
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
    case = dict(cached_case(21, 7, 40, "missing", "clean", 0))
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


@pytest.mark.parametrize("n_inputs, channels, pad", [(3, 7, 5), (33, 2, 1), (64, 3, 16),
                                                     (128, 1, 3), (1, 5, 9)])  # fmt: skip
def test_padding(n_inputs, channels, pad, context, command_queue):
    """Rows padded beyond what the slots ask for, by another amount for every array (so the
    strides differ), and more rows of `pairs`, `iterations` and `status`; run_device checks
    every byte of padding and of the inputs."""
    case = cached_case(40 + pad, channels, n_inputs, "junk", "hostile", 4)
    for variant in ((True, True, True), (False, False, False), (True, False, True)):
        compare(context, command_queue, case, variant, DEFAULT, f"pad {pad}", pad=pad)
    compare(context, command_queue, case, (True, True, True), DEFAULT, f"pad {pad}, in place",
            pad=pad, in_place=True)  # fmt: skip


@pytest.mark.parametrize("channels, n_inputs, extra", [(6, 5, 0), (3, 128, 3), (70, 1, 0),
                                                       (3, 33, 11), (9, 64, 1)])  # fmt: skip
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_inputs, extra, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and an odd stride of its own
    per array; the variants rotate; gains apart from initial and in place."""
    check_raw_abi(offset, channels, n_inputs, extra, context, command_queue)


def check_raw_abi(offset, channels, n_inputs, extra, context, command_queue, views=None,
                  variant=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind; `variant` instead of the one that is due by rotation."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = views or CompactViews(context, queue)
    seed = 31 * offset + n_inputs
    variant = variant or VARIANTS[seed % len(VARIANTS)]
    case = cached_case(seed, channels, n_inputs, gen.TABLES[seed % 5], "hostile", extra)
    given = given_of(case, variant)
    baselines = case["vis"].shape[1]
    fn = host.SolveGainsHost(30, 1e-5, n_inputs - 1, 0x7F, True)
    want = fn(given["vis"], given["pairs"], given["weights"], given["flags"], given["initial"])
    stride_of = {"vis": (baselines + 6) | 1, "weights": (baselines + 2) | 1,
                 "flags": (baselines + 4) | 1, "pairs": (n_inputs + 2) | 1,
                 "initial": (n_inputs + 4) | 1, "gains": (n_inputs + 8) | 1}  # fmt: skip

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    inputs = {name: view(name, value, stride_of[name], True)
              for name, value in given.items() if value is not None and name != "initial"}  # fmt: skip
    mark = views.mark()
    for in_place in (False, True) if given["initial"] is not None else (False,):
        views.release(mark)  # (the arrays of the round before)
        d_initial = None
        if given["initial"] is not None:
            # in place the array is an output: sentinels around it instead of poison
            d_initial = view("gains" if in_place else "initial", given["initial"],
                             stride_of["initial"], not in_place)  # fmt: skip
        if in_place:
            d_gains = d_initial
        else:
            blank = sentinel_array((channels, n_inputs), np.complex64)
            d_gains = view("gains", blank, stride_of["gains"], False)
        d_iterations = view("iterations", sentinel_array((1, channels), np.int32), channels, False)
        d_status = view("status", sentinel_array((1, channels), np.uint8), channels, False)

        def ptr(name):
            return inputs[name][1] if name in inputs else None

        def stride(name):
            return inputs[name][0].stride if name in inputs else 0

        _lib.call("ksp_solve_gains", context.device.index, ctypes.c_void_p(queue.stream),
                  ptr("vis"), ptr("weights"), ptr("flags"), ptr("pairs"),
                  d_initial[1] if d_initial is not None else None, d_gains[1], d_iterations[1],
                  d_status[1], channels, baselines, n_inputs, stride("vis"), stride("weights"),
                  stride("flags"), stride("pairs"),
                  d_initial[0].stride if d_initial is not None else 0, d_gains[0].stride,
                  fn.max_iterations, float(fn.tol2), fn.reference, fn.mask, 1)  # fmt: skip
        # (read asserts that nothing around the rows changed)
        got = (d_gains[0].read("gains"), d_iterations[0].read("iterations")[0],
               d_status[0].read("status")[0])  # fmt: skip
        assert_outputs(want, got, f"at {offset}, in place {in_place}")
        if d_initial is not None and not in_place:
            d_initial[0].read("initial")  # (asserts that nothing wrote to it)
    for name, (d, _) in inputs.items():
        d.read(name)


def test_more_workgroups_than_compute_units(context, command_queue):
    case = cached_case(300, 600, 20, "reversed", "hostile", 2)
    compare(context, command_queue, case, (True, True, False), (30, 1e-3, 0, 0xFF, True),
            "600 channels")  # fmt: skip


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    case = cached_case(11, 5, 12, "reversed", "hostile", 4)
    inputs = gen.inputs_of(case["pairs"], case["vis"].shape[1])
    for variant in VARIANTS:
        template = ingest.SolveGainsTemplate(context, *variant, max_iterations=20, mask=0x0F)
        adapter = ingest.SolveGainsHostFromDevice(template, command_queue)
        given = given_of(case, variant)
        got = adapter(case["vis"], inputs, 12, given["weights"], given["flags"], given["initial"])
        assert_outputs(want_of(case, variant, (20, 1e-5, 0, 0x0F, False)), got, str(variant))


def model_dump(seed, channels, in_baselines, source, ants, truth, unit):
    """int32 (channels, in_baselines, 2): ``g_a conj(g_b)`` of a unit point source plus 1 %
    noise, in units of 1 / `unit`, at the input baselines `source` names; autocorrelations of
    about 8 in the first N_AUTO; noise everywhere else; about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    shape = (channels, in_baselines)
    noise = 0.01 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    vis = noise.copy()
    vis[:, source] += truth[ants[:, 0]] * np.conj(truth[ants[:, 1]])
    vis[:, :N_AUTO] = 8 + noise[:, :N_AUTO].real
    vis_in = np.empty(shape + (2,), np.int32)
    vis_in[..., 0] = np.rint(vis.real * unit)
    vis_in[..., 1] = np.rint(vis.imag * unit)
    lost = rs.random_sample(shape) < 0.03
    lost[:, :N_AUTO] = False
    vis_in[lost, 0] = LOST
    return vis_in


def test_in_the_chain(context, command_queue):
    """Three dumps of model data through prepare -> fused flagger -> accumulate -> finalise ->
    solve -> apply_gains in one sequence, against PrepareHost + FlaggerHost + AveragerHost +
    SolveGainsHost + ApplyGainsHost; the calibrated cross-correlations are the unit source."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, in_baselines, cf, n_inputs = 64, 60, 4, 9
    rs = np.random.RandomState(9)
    cross = np.array(np.triu_indices(n_inputs, 1)).T
    cross = cross[rs.permutation(len(cross))]
    swap = rs.random_sample(len(cross)) < 0.5
    cross[swap] = cross[swap][:, ::-1]
    autos = np.repeat(np.arange(4)[:, np.newaxis], 2, axis=1)
    ants = np.ascontiguousarray(np.concatenate([cross[:20], autos, cross[20:]]), np.int32)
    baselines = len(ants)  # 36 cross-correlations and 4 autocorrelations
    full = device.BackgroundFlags.FULL
    unit = 2.0**17
    scale, lost_flag, weight_scale = 1 / unit, 0x08, 64.0
    prepare = ingest.PrepareTemplate(context, scale, lost_flag, False, True, weight_scale).instantiate(
        queue, channels, baselines, in_baselines)  # fmt: skip
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=full),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    accumulate = device.AccumulateTemplate(context, use_weights=True, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveGainsTemplate(context, max_iterations=60, corrections=True).instantiate(
        queue, channels // cf, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=0x40).instantiate(
        queue, channels // cf, baselines, n_inputs)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "avg_vis": ["finalise:vis", "solve:vis", "apply_gains:vis"],
        "avg_weights": ["finalise:weights", "solve:weights", "apply_gains:weights"],
        "avg_flags": ["finalise:flags", "solve:flags", "apply_gains:flags"],
        "gains": ["solve:gains", "apply_gains:gains"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("solve", solve), ("apply_gains", apply_gains)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is solve.buffer("vis") is apply_gains.buffer("vis")
    assert solve.buffer("gains") is apply_gains.buffer("gains")
    for name in acc:
        seq.buffer(name).zero(queue)
    source = (N_AUTO + rs.permutation(in_baselines - N_AUTO)[:baselines]).astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    truth = gen.make_gains(5, 1, n_inputs, span=1.0)[0].astype(np.complex128)
    pairs = host.SolveGainsHost.pair_table(ants, n_inputs)
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("solve:pairs").set(queue, pairs)
    seq.buffer("apply_gains:inputs").set(queue, ants)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    solve_host = host.SolveGainsHost(max_iterations=60, corrections=True)
    apply_host = host.ApplyGainsHost(0x40)

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, None, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        gains, iterations, status = solve_host(vis, pairs, weights, flags)
        cal_vis, cal_weights, cal_flags = apply_host(vis, gains, ants, weights, flags)
        for name, w in (("avg_vis", vis), ("avg_weights", weights), ("avg_flags", flags),
                        ("gains", gains), ("solve:iterations", iterations),
                        ("solve:status", status), ("apply_gains:out_vis", cal_vis),
                        ("apply_gains:out_weights", cal_weights),
                        ("apply_gains:out_flags", cal_flags)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return gains, status, cal_vis, cal_flags

    for d in range(3):
        vis_in = model_dump(20 + d, channels, in_baselines, source, ants, truth, unit)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        host_dump(vis_in)
    finalise()
    solve()
    apply_gains()
    gains, status, cal_vis, cal_flags = check_outputs()
    # the solution is the model's: converged, and the calibrated cross-correlations are 1
    assert not status.any()
    is_cross = ants[:, 0] != ants[:, 1]
    good = (cal_flags == 0) & is_cross[np.newaxis, :]
    assert good.mean() > 0.7 and np.abs(cal_vis[good] - 1).max() < 0.1
    turned = truth * np.conj(truth[0]) / abs(truth[0])
    assert np.abs(1 / gains - turned[np.newaxis, :]).max() < 0.05
    # and once more through the sequence as a whole
    vis_in = model_dump(40, channels, in_baselines, source, ants, truth, unit)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    check_outputs()
