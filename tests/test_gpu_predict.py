"""Predicting model visibilities on the GPU (``rfi.ingest.PredictTemplate``, ``ksp_predict``):
every comparison is of bit patterns, against ``rfi.host.PredictHost``, with nothing left out but
the payload of a NaN that the host has as a NaN too."""

import ctypes
import functools

import numpy as np
import pytest

from tests import inputs_predict as gen
from tests.inputs_predict import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import LOST, N_AUTO

pytestmark = pytest.mark.gpu

# The sizes at which csrc/predict.hip changes path (ksp_make_tile_geometry, the staging of sources).
# A lane owns a run of RUN baselines and a workgroup has THREADS lanes. A tile is the narrowest
# power of two of runs that holds a row, at most TILE_RUNS = 16 of them: the tile width changes
# at 16, 32, 64, 128 and stays TILE = 256 baselines from there on, so rows beyond 256, 512, ...
# take one more tile. The THREADS / (tile width / RUN) lanes that share a run take different
# rows: 256 rows at once for up to 16 baselines, 16 for 256 and more. Up to BLOCK = 16 sources
# are staged once per workgroup; 17 and more are staged in blocks of 16 for every batch of rows.
RUN = 16
THREADS = 256
TILE = 256
BLOCK = 16

BASELINES = [1, 15, 16, 17, 31, 33, 127, 129, 255, 256, 257, 511, 513]
CHANNELS = [1, 3, 70]
N_SOURCES = [1, 2, 7, 16, 17, 64]
#: (model, divide, weights, flags, in place): model only; divide with and without model,
#: weights and flags; each of those in place
VARIANTS = [(True, False, False, False, False)] + [
    (model, True, weights, flags, in_place)
    for in_place in (False, True) for model in (True, False)
    for weights in (True, False) for flags in (True, False)]  # fmt: skip
NAMES = ("model", "out_vis", "out_weights", "out_flags")
KINDS = ("vis", "weights", "flags")
DTYPES = {"model": np.complex64, "vis": np.complex64, "weights": np.float32, "flags": np.uint8}
f32 = np.float32


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached(seed, channels, baselines, n_sources, pattern="random", flag_value=64):
    """(case, what the host gives for it with every array): every variant's outputs are among
    them, so one reference serves all the variants. Neither is ever modified."""
    from katsdpsigproc_amd.rfi import host

    case = gen.make_case(seed, channels, baselines, n_sources, pattern, flag_value)
    want = host.PredictHost(flag_value)(**case)
    for array in list(case.values()) + list(want):
        array.flags.writeable = False
    return case, dict(zip(NAMES, want))


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, variant, flag_value=64, pad=0):
    """The outputs of the operation by name. The padding of the inputs holds NaN or 0xFF; the
    outputs start out full of sentinel bytes. Afterwards every byte of padding is what it was,
    and so is every byte of the inputs that are not outputs too."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    model, divide, weights, flags, in_place = variant
    channels, (n_sources, baselines) = len(case["freqs"]), case["delays"].shape
    template = ingest.PredictTemplate(context, model, divide, weights, flags, flag_value)
    fn = template.instantiate(queue, channels, baselines, n_sources)
    kinds = [kind for kind, there in zip(KINDS, (divide, weights, flags)) if there]
    for kind in kinds:
        dim = fn.slots[kind].dimensions[1]
        if pad:
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
            out = fn.slots["out_" + kind].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + 2 * pad).link(out)
        if in_place:
            dim.link(fn.slots["out_" + kind].dimensions[1])
    if pad:
        for name in ["delays", "flux"] + (["model"] if model else []):
            dim = fn.slots[name].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + 3 * pad).link(dim)
    fn.ensure_all_bound()
    if in_place:
        fn.bind(**{"out_" + kind: fn.buffer(kind) for kind in kinds})
    uploaded = {}
    for name in ["freqs", "delays", "flux"] + kinds:
        d = fn.buffer(name)
        raw = hostile(d.padded_shape, d.dtype)
        raw[tuple(slice(n) for n in case[name].shape)] = case[name]
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    outputs = (["model"] if model else []) + ["out_" + kind for kind in kinds]
    for name in outputs:
        if not (in_place and name != "model"):
            d = fn.buffer(name)
            queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = {}
    for name in outputs:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        padding = np.ones(d.padded_shape, bool)
        padding[:channels, :baselines] = False
        own = in_place and name != "model"
        before = uploaded[name[4:]] if own else sentinel_array(d.padded_shape, d.dtype)
        same = raw.view(np.uint8) == before.view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out[name] = np.ascontiguousarray(raw[:channels, :baselines])
    for name, before in uploaded.items():
        if in_place and name in kinds:
            continue
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return out


def compare(context, queue, key, variant, pad=0):
    case, want = cached(*key)
    flag_value = key[5] if len(key) > 5 else 64
    got = run_device(context, queue, case, variant, flag_value, pad)
    model, divide, weights, flags, _ = variant
    assert list(got) == [name for name, there in zip(NAMES, (model, divide, weights, flags)) if there]
    for name, g in got.items():
        assert_same(want[name], g, f"{name} of {key}, variant {variant}")
    return want


@pytest.mark.parametrize("variant", VARIANTS)
def test_baselines(variant, context, command_queue):
    """Every width, with the channels, the number of sources and the pattern rotating."""
    for i, baselines in enumerate(BASELINES):
        key = (100 + i, CHANNELS[i % 3], baselines, N_SOURCES[i % 6], gen.PATTERNS[i % 7])
        compare(context, command_queue, key, variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_channels(variant, context, command_queue):
    """Rows around the batches of a workgroup: 256 rows at once at 9 baselines, 64 at 40 and 16
    at 300, where 70 rows are several batches and the last one is ragged."""
    for i, channels in enumerate(CHANNELS):
        for k, baselines in enumerate((9, 40, 300)):
            key = (200 + i, channels, baselines, N_SOURCES[(i + k) % 6], gen.PATTERNS[(i + 2 * k) % 7])
            compare(context, command_queue, key, variant)
    compare(context, command_queue, (210, 257, 9, 3, "random"), variant)


@pytest.mark.parametrize("variant", VARIANTS)
def test_sources(variant, context, command_queue):
    """1 .. 64 sources: one block staged once, and two to four blocks staged per batch."""
    for i, n_sources in enumerate(N_SOURCES):
        for k, (channels, baselines) in enumerate(((5, 300), (40, 33))):
            key = (300 + i, channels, baselines, n_sources, gen.PATTERNS[(i + 3 * k) % 7])
            compare(context, command_queue, key, variant)


@pytest.mark.parametrize("pattern", gen.PATTERNS)
def test_patterns(pattern, context, command_queue):
    """Each pattern on its own at a shape of several tiles and batches, out of place and in
    place, with one block of sources and with two, and with the other flag values."""
    full, in_place = (True, True, True, True, False), (True, True, True, True, True)
    want = compare(context, command_queue, (5, 35, 530, 5, pattern, 1), full)
    compare(context, command_queue, (5, 35, 530, 5, pattern, 1), in_place)
    compare(context, command_queue, (6, 9, 100, 17, pattern, 255), in_place)
    changed = np.mean(want["out_flags"] != cached(5, 35, 530, 5, pattern, 1)[0]["flags"])
    if pattern in ("nonfinite", "flux", "cancel"):
        assert changed > 0.02  # samples that got the bit
    if pattern == "cancel":
        assert (want["out_flags"] & 1).all() and not want["out_weights"].any()
    if pattern in ("random", "large", "exact", "huge"):
        assert changed == 0


@pytest.mark.parametrize("channels, baselines, n_sources, pad", [
    (8, 65, 3, 29), (7, 1025, 16, 3), (5, 256, 17, 16), (3, 257, 64, 35), (70, 15, 2, 40)])  # fmt: skip
def test_padding(channels, baselines, n_sources, pad, context, command_queue):
    """Rows padded beyond what the slots ask for, by a different amount for the inputs, the
    outputs and delays, flux and model (so the strides differ); run_device checks every byte
    of padding and of the inputs."""
    for variant in VARIANTS[::2] + VARIANTS[-1:]:
        compare(context, command_queue, (pad, channels, baselines, n_sources, "nonfinite"),
                variant, pad=pad)  # fmt: skip


def odd_strides(baselines, n_sources):
    """delays, flux, then model, vis, weights, flags, out_vis, out_weights, out_flags"""
    return (baselines + 4) | 1, (n_sources + 2) | 1, [(baselines + k) | 1 for k in (14, 6, 2, 4, 8, 10, 12)]


def aligned_strides(baselines, n_sources):
    whole = -(-baselines // 16) * 16
    return baselines + 3, n_sources + 1, [whole + 16 * k for k in (2, 1, 2, 1, 3, 1, 2)]


@pytest.mark.parametrize("channels, baselines, n_sources", [
    (6, 37, 5), (3, 259, 17), (70, 1, 1), (3, 15, 64), (3, 16, 16), (3, 17, 2), (9, 33, 7)])  # fmt: skip
@pytest.mark.parametrize("offset, strides", [(1, odd_strides), (4, odd_strides), (12, odd_strides),
                                             (16, aligned_strides), (4, aligned_strides)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, channels, baselines, n_sources, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and a stride of its own per
    array, delays and flux included. Odd strides and offsets of 1, 4 and 12 elements take the
    element-wise path; 16 elements and strides that keep the rows on 16 bytes take the 16-byte
    path from the middle of an allocation; 4 elements with such strides leave the flags off 16
    bytes. The variants rotate; in place and out of place both."""
    check_raw_abi(offset, strides, channels, baselines, n_sources, context, command_queue)


def check_raw_abi(offset, strides, channels, baselines, n_sources, context, command_queue,
                  views=None, variant=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind; `variant` instead of the one that is due by rotation."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = views or CompactViews(context, queue)
    seed = 31 * offset + baselines
    model, divide, weights, flags, _ = variant or VARIANTS[seed % 9]
    case, want = cached(seed, channels, baselines, n_sources, gen.PATTERNS[seed % 7])
    delays_stride, flux_stride, data_strides = strides(baselines, n_sources)
    kinds = [kind for kind, there in zip(KINDS, (divide, weights, flags)) if there]
    stride_of = dict(zip(("model",) + KINDS + tuple("out_" + kind for kind in KINDS), data_strides))

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    d_freqs = view("freqs", case["freqs"][np.newaxis, :], channels, True)
    d_delays = view("delays", case["delays"], delays_stride, True)
    d_flux = view("flux", case["flux"], flux_stride, True)
    mark = views.mark()
    for in_place in (False, True) if divide else (False,):
        views.release(mark)  # (the arrays of the round before)
        d_in, d_out = {}, {}
        if model:
            blank = sentinel_array((channels, baselines), np.complex64)
            d_out["model"] = view("model", blank, stride_of["model"], False)
        for kind in kinds:
            # in place the array is an output: sentinels around it instead of poison
            d_in[kind] = view(("out_" if in_place else "") + kind, case[kind], stride_of[kind],
                              not in_place)  # fmt: skip
            if in_place:
                d_out[kind] = d_in[kind]
            else:
                blank = sentinel_array((channels, baselines), DTYPES[kind])
                d_out[kind] = view("out_" + kind, blank, stride_of["out_" + kind], False)

        def ptr(views, kind):
            return views[kind][1] if kind in views else None

        def stride(views, kind):
            return views[kind][0].stride if kind in views else 0

        _lib.call("ksp_predict", context.device.index, ctypes.c_void_p(queue.stream),
                  d_freqs[1], d_delays[1], d_flux[1], ptr(d_out, "model"), ptr(d_in, "vis"),
                  ptr(d_in, "weights"), ptr(d_in, "flags"), ptr(d_out, "vis"),
                  ptr(d_out, "weights"), ptr(d_out, "flags"), channels, baselines, n_sources,
                  d_delays[0].stride, d_flux[0].stride, stride(d_out, "model"), stride(d_in, "vis"),
                  stride(d_in, "weights"), stride(d_in, "flags"), stride(d_out, "vis"),
                  stride(d_out, "weights"), stride(d_out, "flags"), 64)  # fmt: skip
        what = f"at {offset}, in place {in_place}"
        if model:
            assert_same(want["model"], d_out["model"][0].read("model"), "model " + what)
        for kind in kinds:
            got = d_out[kind][0].read("out_" + kind)  # (asserts that nothing around it changed)
            assert_same(want["out_" + kind], got, f"out_{kind} {what}")
            if not in_place:
                d_in[kind][0].read(kind)  # (asserts that nothing wrote to it)
    d_freqs[0].read("freqs")
    d_delays[0].read("delays")
    d_flux[0].read("flux")


def test_many_workgroups_and_chunks(context, command_queue):
    key = (300, 300, 5000, 3, "flux")
    compare(context, command_queue, key, (True, True, True, True, True))
    compare(context, command_queue, key, (False, True, True, True, True))


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    case, want = cached(11, 12, 70, 9, "nonfinite", 2)
    for model, divide, weights, flags, in_place in VARIANTS:
        if in_place:
            continue
        template = ingest.PredictTemplate(context, model, divide, weights, flags, flag_value=2)
        adapter = ingest.PredictHostFromDevice(template, command_queue)
        got = adapter(case["freqs"], case["delays"], case["flux"],
                      case["vis"] if divide else None, case["weights"] if weights else None,
                      case["flags"] if flags else None)  # fmt: skip
        for name, there, g in zip(NAMES, (model, divide, weights, flags), got):
            assert (g is not None) == there, name
            if there:
                assert_same(want[name], g, name)


def field_dump(seed, in_baselines, source, ants, truth, field, unit):
    """int32 (channels, in_baselines, 2): ``g_a conj(g_b) M`` plus 1 % noise, in units of
    1 / `unit`, at the input baselines `source` names, where ``M = field[c]`` (channels x
    baselines) is the model of every unaveraged channel; autocorrelations of about 8 in the
    first N_AUTO; noise everywhere else; about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    shape = (len(field), in_baselines)
    noise = 0.01 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    vis = noise.copy()
    vis[:, source] += truth[ants[:, 0]] * np.conj(truth[ants[:, 1]]) * field
    vis[:, :N_AUTO] = 8 + noise[:, :N_AUTO].real
    vis_in = np.empty(shape + (2,), np.int32)
    vis_in[..., 0] = np.rint(vis.real * unit)
    vis_in[..., 1] = np.rint(vis.imag * unit)
    lost = rs.random_sample(shape) < 0.03
    lost[:, :N_AUTO] = False
    vis_in[lost, 0] = LOST
    return vis_in


def test_in_the_chain(context, command_queue):
    """Three dumps of a three-source field through prepare -> fused flagger -> accumulate ->
    finalise -> predict (divide) -> solve -> apply_gains in one sequence, against PrepareHost +
    FlaggerHost + AveragerHost + PredictHost + SolveGainsHost + ApplyGainsHost in the same
    order. apply_gains reads what finalise left, so the calibrated cross-correlations are the
    model, not 1."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest
    from tests import inputs_solve_gains as gen_solve

    queue = command_queue
    channels, in_baselines, cf, n_inputs, n_sources = 64, 60, 4, 9, 3
    rows = channels // cf
    rs = np.random.RandomState(9)
    cross = np.array(np.triu_indices(n_inputs, 1)).T
    cross = cross[rs.permutation(len(cross))]
    swap = rs.random_sample(len(cross)) < 0.5
    cross[swap] = cross[swap][:, ::-1]
    autos = np.repeat(np.arange(4)[:, np.newaxis], 2, axis=1)
    ants = np.ascontiguousarray(np.concatenate([cross[:20], autos, cross[20:]]), np.int32)
    baselines = len(ants)  # 36 cross-correlations and 4 autocorrelations
    positions = rs.uniform(-400, 400, (n_inputs, 3)) * [1, 1, 0.02]
    uvw = positions[ants[:, 0]] - positions[ants[:, 1]]
    lm = np.array([[0.0, 0.0], [0.004, -0.003], [-0.002, 0.005]])
    delays = host.PredictHost.delays(uvw, lm)
    fine_freqs = np.linspace(1.3e9, 1.5e9, channels)
    freqs = fine_freqs.reshape(rows, cf).mean(axis=1)
    brightness = np.array([[1.0, 0.5, 0.3]])
    flux = (brightness * (freqs[:, np.newaxis] / 1.4e9) ** -0.7).astype(f32)
    fine_flux = (brightness * (fine_freqs[:, np.newaxis] / 1.4e9) ** -0.7).astype(f32)
    field = host.PredictHost()(freqs, delays, flux)[0]
    fine_field = host.PredictHost()(fine_freqs, delays, fine_flux)[0]
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
    predict = ingest.PredictTemplate(context, model=False, divide=True, flag_value=0x20).instantiate(
        queue, rows, baselines, n_sources)  # fmt: skip
    solve = ingest.SolveGainsTemplate(context, max_iterations=60, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=0x40).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "gains": ["solve:gains", "apply_gains:gains"],
    }
    for kind in KINDS:
        compounds["avg_" + kind] = ["finalise:" + kind, "predict:" + kind, "apply_gains:" + kind]
        compounds["unit_" + kind] = ["predict:out_" + kind, "solve:" + kind]
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("predict", predict), ("solve", solve),
                ("apply_gains", apply_gains)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is predict.buffer("vis") is apply_gains.buffer("vis")
    assert predict.buffer("out_vis") is solve.buffer("vis")
    assert predict.buffer("out_vis") is not predict.buffer("vis")
    assert solve.buffer("gains") is apply_gains.buffer("gains")
    for name in acc:
        seq.buffer(name).zero(queue)
    source = (N_AUTO + rs.permutation(in_baselines - N_AUTO)[:baselines]).astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    truth = gen_solve.make_gains(5, 1, n_inputs, span=1.0)[0].astype(np.complex128)
    pairs = host.SolveGainsHost.pair_table(ants, n_inputs)
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("predict:freqs").set(queue, freqs)
    seq.buffer("predict:delays").set(queue, delays)
    seq.buffer("predict:flux").set(queue, flux)
    seq.buffer("solve:pairs").set(queue, pairs)
    seq.buffer("apply_gains:inputs").set(queue, ants)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    predict_host = host.PredictHost(0x20)
    solve_host = host.SolveGainsHost(max_iterations=60, corrections=True)
    apply_host = host.ApplyGainsHost(0x40)

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, None, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        _, unit_vis, unit_weights, unit_flags = predict_host(freqs, delays, flux, vis, weights, flags)
        gains, iterations, status = solve_host(unit_vis, pairs, unit_weights, unit_flags)
        cal_vis, cal_weights, cal_flags = apply_host(vis, gains, ants, weights, flags)
        for name, w in (("avg_vis", vis), ("avg_weights", weights), ("avg_flags", flags),
                        ("unit_vis", unit_vis), ("unit_weights", unit_weights),
                        ("unit_flags", unit_flags), ("gains", gains),
                        ("solve:iterations", iterations), ("solve:status", status),
                        ("apply_gains:out_vis", cal_vis), ("apply_gains:out_weights", cal_weights),
                        ("apply_gains:out_flags", cal_flags)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return gains, status, cal_vis, cal_flags

    def dump(seed):
        return field_dump(seed, in_baselines, source, ants, truth, fine_field, unit)

    for d in range(3):
        vis_in = dump(20 + d)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        host_dump(vis_in)
    finalise()
    predict()
    solve()
    apply_gains()
    gains, status, cal_vis, cal_flags = check_outputs()
    # the solution is the true gains: converged, and the calibrated cross-correlations are the
    # field as the sky has it, which is far from a unit source
    assert not status.any()
    is_cross = ants[:, 0] != ants[:, 1]
    good = (cal_flags == 0) & is_cross[np.newaxis, :]
    assert good.mean() > 0.7 and np.abs(cal_vis[good] - field[good]).max() < 0.1
    assert np.abs(field[good] - 1).max() > 0.5
    turned = truth * np.conj(truth[0]) / abs(truth[0])
    assert np.abs(1 / gains - turned[np.newaxis, :]).max() < 0.05
    # and once more through the sequence as a whole
    vis_in = dump(40)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    check_outputs()
