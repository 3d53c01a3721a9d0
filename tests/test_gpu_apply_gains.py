"""Applying gains on the GPU (``rfi.ingest.ApplyGainsTemplate``, ``ksp_apply_gains``): every
comparison is of bit patterns, against ``rfi.host.ApplyGainsHost``, with nothing left out but
the payload of a NaN that the host has as a NaN too."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests import inputs_apply_gains as gen
from tests.inputs_apply_gains import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import N_AUTO, chain_dump

pytestmark = pytest.mark.gpu

# The sizes at which csrc/apply_gains.hip changes path (ksp_make_tile_geometry, ag_stage_rows).
# A lane owns a run of RUN baselines and a workgroup has THREADS lanes. A tile is the narrowest
# power of two of runs that holds a row, at most THREADS of them: the tile width changes at
# 16, 32, 64, ... and stays TILE = 4096 baselines from there on, so rows beyond 4096, 8192, ...
# take one more tile. The THREADS / (tile width / RUN) lanes that share a run take different
# rows. A stage holds stage_rows(n_inputs) rows of gains in LDS_GAINS = 4096 slots of 8 bytes;
# a workgroup's chunk of rows is at least THREADS / (tile width / RUN) rows (256 rows for up to
# 16 baselines, 64 for up to 64), so with narrow arrays a workgroup walks several stages.
RUN = 16
THREADS = 256
TILE = RUN * THREADS
LDS_GAINS = 4096
TILE_WIDTHS = [RUN << k for k in range(9)]  # 16 .. 4096


def stage_rows(n_inputs):
    return min(THREADS, LDS_GAINS // n_inputs)


BASELINES = sorted(
    {1, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097}
    | {width + d for width in TILE_WIDTHS + [2 * TILE] for d in (-1, 0, 1)})  # fmt: skip
CHANNELS = [1, 2, 7, 8]
N_INPUTS = [1, 2, 3, 64, 65, 128, 4095, 4096]
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]
NAMES = ("out_vis", "out_weights", "out_flags")
DTYPES = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}
f32 = np.float32


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def want_of(case, weights, flags, flag_value=128):
    from katsdpsigproc_amd.rfi import host

    return host.ApplyGainsHost(flag_value)(
        case["vis"], case["gains"], case["inputs"], case["weights"] if weights else None,
        case["flags"] if flags else None)  # fmt: skip


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, weights, flags, in_place, flag_value=128, pad=0):
    """(out_vis, out_weights or None, out_flags or None) of the operation. The padding of the
    inputs holds NaN or 0xFF; the outputs start out full of sentinel bytes. Afterwards every
    byte of padding is what it was, and out of place so is every byte of the inputs."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    channels, baselines = case["vis"].shape
    n_inputs = case["gains"].shape[1]
    template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags, flag_value=flag_value)
    fn = template.instantiate(queue, channels, baselines, n_inputs)
    kinds = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
    for kind in kinds:
        dim = fn.slots[kind].dimensions[1]
        if pad:
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
            out = fn.slots["out_" + kind].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + 2 * pad).link(out)
        if in_place:
            dim.link(fn.slots["out_" + kind].dimensions[1])
    if pad:
        dim = fn.slots["gains"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    if in_place:
        fn.bind(**{"out_" + kind: fn.buffer(kind) for kind in kinds})
    uploaded = {}
    for name in kinds + ["gains", "inputs"]:
        d = fn.buffer(name)
        width = case[name].shape[1]
        assert d.padded_shape[1] >= width + (pad if name != "inputs" else 0)
        raw = hostile(d.padded_shape, d.dtype)
        raw[: case[name].shape[0], :width] = case[name]
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    if not in_place:
        for kind in kinds:
            d = fn.buffer("out_" + kind)
            queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = {}
    for kind in kinds:
        d = fn.buffer("out_" + kind)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        padding = np.ones(d.padded_shape, bool)
        padding[:channels, :baselines] = False
        before = uploaded[kind] if in_place else sentinel_array(d.padded_shape, d.dtype)
        same = raw.view(np.uint8) == before.view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=1)].all(), \
            f"wrote into the padding of out_{kind}"  # fmt: skip
        out[kind] = np.ascontiguousarray(raw[:channels, :baselines])
    for name, before in uploaded.items():
        if in_place and name in kinds:
            continue
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return out["vis"], out.get("weights"), out.get("flags")


def compare(context, queue, case, weights, flags, in_place, what, flag_value=128, pad=0):
    want = want_of(case, weights, flags, flag_value)
    got = run_device(context, queue, case, weights, flags, in_place, flag_value, pad)
    for name, w, g in zip(NAMES, want, got):
        assert (w is None) == (g is None), name
        if w is not None:
            assert_same(w, g, f"{name} {what}")
    return want


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_baselines(weights, flags, in_place, context, command_queue):
    """Every width, with the channels, the number of inputs and the index pattern rotating."""
    for i, baselines in enumerate(BASELINES):
        channels = CHANNELS[i % len(CHANNELS)]
        n_inputs = N_INPUTS[(i // 2) % len(N_INPUTS)]
        pattern = gen.PATTERNS[i % len(gen.PATTERNS)]
        case = gen.make_case(1000 * i + baselines, channels, baselines, n_inputs, pattern)
        compare(context, command_queue, case, weights, flags, in_place,
                f"{channels}x{baselines}, {n_inputs} inputs, {pattern}")  # fmt: skip


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_stages(n_inputs, context, command_queue):
    """Rows around the end of a stage and of a workgroup's chunk, for arrays narrow enough that
    a chunk holds several stages (5 and 40 baselines: chunks of 256 and 64 rows) and one that
    is not (300: 8 rows)."""
    rows = stage_rows(n_inputs)
    assert rows == {1: 256, 2: 256, 3: 256, 64: 64, 65: 63, 128: 32, 4095: 1, 4096: 1}[n_inputs]
    channels_list = sorted(set(CHANNELS) | {max(rows + d, 1) for d in (-1, 0, 1)}
                           | {2 * rows + 1, 63, 64, 65, 255, 256, 257})  # fmt: skip
    all_gains = gen.make_gains(n_inputs, channels_list[-1], n_inputs)
    for i, channels in enumerate(channels_list):
        for baselines in (5, 40, 300):
            weights, flags = VARIANTS[i % 4]
            pattern = gen.PATTERNS[(i + baselines) % len(gen.PATTERNS)]
            seed = 77 * channels + baselines
            case = {"vis": gen.make_vis(seed, channels, baselines),
                    # (the last rows, so that the rows of a stage differ from shape to shape)
                    "gains": np.ascontiguousarray(all_gains[-channels:]),
                    "inputs": gen.make_inputs(seed, pattern, baselines, n_inputs),
                    "weights": gen.make_weights(seed, channels, baselines),
                    "flags": gen.make_flags(seed, channels, baselines)}  # fmt: skip
            compare(context, command_queue, case, weights, flags, bool(i % 2),
                    f"{channels}x{baselines}, {n_inputs} inputs, {pattern}")  # fmt: skip


@pytest.mark.parametrize("pattern", gen.PATTERNS)
def test_patterns(pattern, context, command_queue):
    """Each index pattern on its own at a shape of several tiles and stages, and with the
    other flag values."""
    case = gen.make_case(5, 70, 4200, 128, pattern, flag_value=1)
    assert (case["flags"] & 1).any()
    want = compare(context, command_queue, case, True, True, False, pattern, flag_value=1)
    assert np.mean(want[2] != case["flags"]) > 0.02  # samples that got the bit
    case = gen.make_case(6, 9, 100, 4096, pattern, flag_value=255)
    compare(context, command_queue, case, True, True, True, pattern, flag_value=255)


@pytest.mark.parametrize("channels, baselines, n_inputs, pad", [
    (8, 65, 3, 29), (7, 1025, 64, 3), (5, 256, 128, 16), (3, TILE + 1, 65, 35), (70, 15, 2, 40)])  # fmt: skip
@pytest.mark.parametrize("in_place", [False, True])
def test_padding(channels, baselines, n_inputs, pad, in_place, context, command_queue):
    """Rows padded beyond what the slots ask for, `pad` elements for the inputs and the gains
    and twice that for the outputs (so the strides differ); run_device checks every byte of
    padding and, out of place, of the inputs."""
    case = gen.make_case(pad, channels, baselines, n_inputs, "outside")
    for weights, flags in VARIANTS:
        compare(context, command_queue, case, weights, flags, in_place, f"pad {pad}", pad=pad)


def odd_strides(baselines, n_inputs):
    return [(baselines + k) | 1 for k in (6, 2, 4, 8, 10, 12)], (n_inputs + 2) | 1


def aligned_strides(baselines, n_inputs):
    return [-(-baselines // 16) * 16 + 16 * k for k in (1, 2, 1, 3, 1, 2)], n_inputs + 2 & ~1


@pytest.mark.parametrize("channels, baselines, n_inputs", [
    (6, 37, 5), (3, TILE + 3, 128), (70, 1, 1), (3, 15, 64), (3, 16, 4096), (3, 17, 2), (9, 33, 65)])  # fmt: skip
@pytest.mark.parametrize("offset, strides", [(1, odd_strides), (4, odd_strides), (12, odd_strides),
                                             (16, aligned_strides), (4, aligned_strides)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, channels, baselines, n_inputs, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and a stride of its own per
    array. Odd strides and offsets of 1, 4 and 12 elements take the element-wise path; 16
    elements and strides that keep the rows on 16 bytes take the 16-byte path from the middle
    of an allocation; 4 elements with such strides leave the flags off 16 bytes. The variants
    rotate; in place and out of place both."""
    check_raw_abi(offset, strides, channels, baselines, n_inputs, context, command_queue)


def check_raw_abi(offset, strides, channels, baselines, n_inputs, context, command_queue,
                  views=None, variant=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind; `variant` instead of the one that is due by rotation."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = views or CompactViews(context, queue)
    seed = 31 * offset + baselines
    weights, flags = variant or VARIANTS[seed % 4]
    case = gen.make_case(seed, channels, baselines, n_inputs, gen.PATTERNS[seed % 5])
    data_strides, gains_stride = strides(baselines, n_inputs)
    want = want_of(case, weights, flags)
    kinds = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
    stride_of = dict(zip(("vis", "weights", "flags", "out_vis", "out_weights", "out_flags"),
                         data_strides))  # fmt: skip

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    d_gains = view("gains", case["gains"], gains_stride, True)
    d_inputs = view("inputs", case["inputs"], 2, True)
    mark = views.mark()
    for in_place in (False, True):
        views.release(mark)  # (the arrays of the round before)
        d_in, d_out = {}, {}
        for kind in kinds:
            # in place the array is an output: sentinels around it instead of poison
            d_in[kind] = view(kind, case[kind], stride_of[kind], not in_place)
            if in_place:
                d_out[kind] = d_in[kind]
            else:
                blank = sentinel_array((channels, baselines), DTYPES[kind])
                d_out[kind] = view("out_" + kind, blank, stride_of["out_" + kind], False)

        def ptr(views, kind):
            return views[kind][1] if kind in views else None

        def stride(views, kind):
            return views[kind][0].stride if kind in views else 0

        _lib.call("ksp_apply_gains", context.device.index, ctypes.c_void_p(queue.stream),
                  ptr(d_in, "vis"), ptr(d_in, "weights"), ptr(d_in, "flags"), d_gains[1],
                  d_inputs[1], ptr(d_out, "vis"), ptr(d_out, "weights"), ptr(d_out, "flags"),
                  channels, baselines, n_inputs, stride(d_in, "vis"), stride(d_in, "weights"),
                  stride(d_in, "flags"), d_gains[0].stride, stride(d_out, "vis"),
                  stride(d_out, "weights"), stride(d_out, "flags"), 128)  # fmt: skip
        for kind, w in zip(("vis", "weights", "flags"), want):
            if kind in kinds:
                got = d_out[kind][0].read("out_" + kind)  # (asserts that nothing around it changed)
                assert_same(w, got, f"out_{kind} at {offset}, in place {in_place}")
                if not in_place:
                    d_in[kind][0].read(kind)  # (asserts that nothing wrote to it)
    d_gains[0].read("gains")
    d_inputs[0].read("inputs")


def test_many_workgroups_and_stages(context, command_queue):
    case = gen.make_case(300, 300, 5000, 128, "outside")
    compare(context, command_queue, case, True, True, False, "300x5000")
    compare(context, command_queue, case, True, True, True, "300x5000 in place")


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    case = gen.make_case(11, 12, 70, 9, "outside")
    for weights, flags in VARIANTS:
        template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags, flag_value=2)
        adapter = ingest.ApplyGainsHostFromDevice(template, command_queue)
        got = adapter(case["vis"], case["gains"], case["inputs"],
                      case["weights"] if weights else None, case["flags"] if flags else None)  # fmt: skip
        for name, w, g in zip(NAMES, want_of(case, weights, flags, 2), got):
            assert (w is None) == (g is None)
            if w is not None:
                assert_same(w, g, name)


def test_in_the_chain(context, command_queue):
    """Three dumps through prepare -> fused flagger -> accumulate -> finalise -> apply_gains ->
    compress in one sequence, against PrepareHost + FlaggerHost + AveragerHost + ApplyGainsHost
    + CompressWeightsHost; the averaged output stays as finalise left it."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, in_baselines, cf, n_inputs = 64, 40, 50, 4, 9
    full = device.BackgroundFlags.FULL
    scale, lost_flag, weight_scale = 2.0**-8, 0x08, 2.0**24
    prepare = ingest.PrepareTemplate(context, scale, lost_flag, True, True, weight_scale).instantiate(
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
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=0x40).instantiate(
        queue, channels // cf, baselines, n_inputs)  # fmt: skip
    compress = ingest.CompressWeightsTemplate(context).instantiate(queue, channels // cf, baselines)
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "avg_vis": ["finalise:vis", "apply_gains:vis"],
        "avg_weights": ["finalise:weights", "apply_gains:weights"],
        "avg_flags": ["finalise:flags", "apply_gains:flags"],
        "cal_weights": ["apply_gains:out_weights", "compress:weights"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("apply_gains", apply_gains), ("compress", compress)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("weights") is apply_gains.buffer("weights")
    assert apply_gains.buffer("out_weights") is compress.buffer("weights")
    for name in acc:
        seq.buffer(name).zero(queue)
    rs = np.random.RandomState(9)
    source = rs.permutation(in_baselines)[:baselines].astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    mask = inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * np.uint8(0x20)
    gains = gen.make_gains(3, channels // cf, n_inputs, special=False)
    gains = (gains / np.abs(gains) * rs.uniform(0.5, 2, gains.shape)).astype(np.complex64)
    gains[3, 2] = complex(np.nan, 0)  # no solution for input 2 in one channel
    gains[:, 7] = 0  # an input that is switched off
    ants = gen.make_inputs(8, "random", baselines, n_inputs)
    ants[5] = (n_inputs, 0)  # a baseline of an input that has no gains at all
    ants[6] = (4, 4)
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("prepare:channel_flags").set(queue, mask)
    seq.buffer("apply_gains:gains").set(queue, gains)
    seq.buffer("apply_gains:inputs").set(queue, ants)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    apply_host = host.ApplyGainsHost(0x40)
    compress_host = host.CompressWeightsHost()

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, mask, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        cal_vis, cal_weights, cal_flags = apply_host(vis, gains, ants, weights, flags)
        weights8, weights_channel = compress_host(cal_weights)
        for name, w in (("avg_vis", vis), ("avg_weights", weights), ("avg_flags", flags),
                        ("apply_gains:out_vis", cal_vis), ("cal_weights", cal_weights),
                        ("apply_gains:out_flags", cal_flags), ("compress:weights8", weights8),
                        ("compress:weights_channel", weights_channel)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return vis, cal_vis, cal_weights, cal_flags

    for d in range(3):
        vis_in = chain_dump(20 + d, channels, in_baselines)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        host_dump(vis_in)
    finalise()
    apply_gains()
    compress()
    vis, cal_vis, cal_weights, cal_flags = check_outputs()
    # the corrections did something, and the samples without one are as the definition says
    assert np.mean(cal_vis != vis) > 0.5
    uses2 = (ants == 2).any(axis=1)
    assert uses2.any() and (cal_flags[3, uses2] & 0x40).all() and not cal_weights[3, uses2].any()
    assert (cal_flags[:, 5] & 0x40).all() and not (cal_flags[:, 6] & 0x40).any()
    assert not cal_weights[:, (ants == 7).any(axis=1)].any()
    g4 = gains[:, 4]  # baseline 6 is its autocorrelation: ci = +0, cr = |g4|^2
    assert (cal_vis[:, 6].imag == vis[:, 6].imag * (g4.real * g4.real + g4.imag * g4.imag)).all()
    # and once more through the sequence as a whole
    vis_in = chain_dump(40, channels, in_baselines)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    check_outputs()
