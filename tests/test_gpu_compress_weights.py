"""Compressing weights on the GPU (``rfi.ingest.CompressWeightsTemplate``,
``ksp_compress_weights``): every comparison is of bit patterns, against
``rfi.host.CompressWeightsHost``, with nothing left out."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests.subviews import SENTINEL, CompactViews, flat_device_array, sentinel_array

pytestmark = pytest.mark.gpu

# The row lengths at which csrc/compress_weights.hip changes path (cw_path): up to WAVE_MAX a
# wavefront per row (four rows per workgroup), up to SMALL_MAX four wavefronts, up to MEDIUM_MAX
# sixteen, up to RESIDENT_MAX sixteen with two runs of 16 baselines per lane; that is the
# register-resident limit, and longer rows are read twice.
WAVE_MAX = 1024
SMALL_MAX = 4096
MEDIUM_MAX = 16384
RESIDENT_MAX = 32768
PATH_LIMITS = [WAVE_MAX, SMALL_MAX, MEDIUM_MAX, RESIDENT_MAX]
BASELINES = sorted(
    {1, 3, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097}
    | {limit + d for limit in PATH_LIMITS for d in (-1, 0, 1)})  # fmt: skip
CHANNELS = [1, 2, 7, 8]
RUN = 16  # baselines of a 16-byte store
f32 = np.float32
TINY = f32(2.0**-149)
HUGE = f32(2.0**127)  # finite and positive: a kernel that reads it corrupts the maximum

ROW_KINDS = ["mix", "ties", "mix", "denormal", "mix", "zero", "inf", "mix"]
N_PLACES = 5


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def place(choice, baselines, rs):
    """The column of a row's maximum: 0, the last, the last of the part that goes in whole
    16-byte stores, the first of the ragged tail, a random one."""
    whole = baselines // RUN * RUN
    return [0, baselines - 1, max(whole - 1, 0), min(whole, baselines - 1),
            int(rs.randint(baselines))][choice]  # fmt: skip


def make_row(rs, kind, baselines):
    """(one row without its maximum, the maximum to give it or None for twice its largest
    positive finite weight); every positive finite value is at most 2^30."""
    if kind == "zero":
        return np.where(rs.random_sample(baselines) < 0.5, f32(0), f32(-0.0)), None
    if kind == "inf":
        return np.full(baselines, np.inf, f32), None
    if kind == "denormal":  # k 2^-149, k < 2^20: twice the largest is still a denormal
        row = (rs.randint(1, 2**20, baselines) * np.float64(TINY)).astype(f32)
        row[rs.random_sample(baselines) < 0.1] = 0
        return row, None
    if kind == "ties":  # (k + 0.5) 2^e against a maximum of 255 2^e: t = k + 0.5 exactly
        e = int(rs.randint(-20, 21))
        row = ((rs.randint(1, 127, baselines) + 0.5) * 2.0**e).astype(f32)
        row[rs.random_sample(baselines) < 0.1] = 0
        return row, f32(255 * 2.0**e)
    row = np.exp2(rs.uniform(-30, 30, baselines)).astype(f32)
    what = rs.random_sample(baselines)
    row[what < 0.10] = 0
    for i, value in enumerate([np.nan, np.inf, -np.inf, -2.5, -0.0, TINY, 2.0**-130, 1e-40]):
        row[(what >= 0.10 + 0.015 * i) & (what < 0.115 + 0.015 * i)] = value
    return row, None


DISTINCT_ROWS = 64


def make_weights(seed, channels, baselines, rotation=0):
    """float32 (channels, baselines), and the column of each row's maximum (-1: the row has
    none). The kind of a row and the place of its maximum rotate with the row; the maximum
    stands alone, with every other positive finite weight of the row at most half of it.
    Beyond DISTINCT_ROWS rows the rows repeat, block k of them scaled by 2^(k % 8)."""
    rs = np.random.RandomState(seed)
    distinct = min(channels, DISTINCT_ROWS)
    weights = np.empty((distinct, baselines), f32)
    columns = np.full(distinct, -1)
    for c in range(distinct):
        kind = ROW_KINDS[(c + rotation) % len(ROW_KINDS)]
        row, peak = make_row(rs, kind, baselines)
        if kind not in ("zero", "inf"):
            col = place((c + rotation) % N_PLACES, baselines, rs)
            row[col] = 0
            ok = (row > 0) & (row < np.inf)
            if peak is None:
                peak = f32(2) * row[ok].max() if ok.any() else f32(0.5)
            row[col] = peak
            columns[c] = col
        weights[c] = row
    if channels > distinct:
        blocks = -(-channels // distinct)
        factor = np.exp2(np.arange(blocks) % 8).astype(f32).repeat(distinct)[:channels]
        weights = np.tile(weights, (blocks, 1))[:channels] * factor[:, np.newaxis]
        columns = np.tile(columns, blocks)[:channels]
    return weights, columns


def ties_rows(seed, channels, baselines):
    """Rows of exact ties alone: a maximum of 255 2^e at a rotating place, every other weight
    (k + 0.5) 2^e with k = 1 .. 126, so t = k + 0.5 exactly and rint rounds to even."""
    rs = np.random.RandomState(seed)
    weights = np.empty((channels, baselines), f32)
    for c in range(channels):
        e = int(rs.randint(-20, 21))
        weights[c] = (((np.arange(baselines) + c) % 126 + 1.5) * 2.0**e).astype(f32)
        weights[c, place(c % N_PLACES, baselines, rs)] = 255 * 2.0**e
    return weights


def assert_same(want, got, what=""):
    assert want.dtype == got.dtype and want.shape == got.shape, what
    if want.dtype == np.uint8:
        bad = want != got
        assert not bad.any(), (
            f"{what}: {np.count_nonzero(bad)} of {bad.size} bytes differ, first at "
            f"{np.argwhere(bad)[0]}: want {want[bad][0]}, got {got[bad][0]}")  # fmt: skip
        return
    want = np.ascontiguousarray(want).view(np.uint32)
    got = np.ascontiguousarray(got).view(np.uint32)
    bad = want != got
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ, first at "
        f"{np.argwhere(bad)[0]}: want {want[bad][0]:#010x}, got {got[bad][0]:#010x}")  # fmt: skip


def hostile_padding(shape):
    """What the padding of `weights` holds: 2^127 and NaN in turn."""
    raw = np.full(shape, HUGE, f32)
    raw.reshape(-1)[1::2] = np.nan
    return raw


def run_device(context, queue, weights, pad=0):
    """(weights8, weights_channel) of the operation. The padding of `weights` holds 2^127 and
    NaN; `weights8` starts out full of sentinel bytes, and its padding is checked afterwards."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    channels, baselines = weights.shape
    fn = ingest.CompressWeightsTemplate(context).instantiate(queue, channels, baselines)
    if pad:
        for name in ("weights", "weights8"):
            dim = fn.slots[name].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    d_weights, d_weights8 = fn.buffer("weights"), fn.buffer("weights8")
    assert d_weights.padded_shape[1] >= baselines + pad
    assert d_weights8.padded_shape[1] >= baselines + pad
    raw = hostile_padding(d_weights.padded_shape)
    raw[:, :baselines] = weights
    queue.enqueue_write_buffer(d_weights.buffer, raw)
    queue.enqueue_write_buffer(d_weights8.buffer, sentinel_array(d_weights8.padded_shape, np.uint8))
    fn.buffer("weights_channel").set(queue, np.full(channels, -1, f32))
    fn()
    raw8 = np.empty(d_weights8.padded_shape, np.uint8)
    queue.enqueue_read_buffer(d_weights8.buffer, raw8)
    assert np.all(raw8[:, baselines:] == SENTINEL), "wrote into the padding of weights8"
    return np.ascontiguousarray(raw8[:, :baselines]), fn.buffer("weights_channel").get(queue)


def compare(context, queue, weights, what, columns=None, pad=0):
    from katsdpsigproc_amd.rfi import host

    want = host.CompressWeightsHost()(weights)
    if columns is not None:
        # the reference itself: the scale of a row is its marked weight over 255
        for c, col in enumerate(columns):
            if col >= 0:
                assert want[1][c] == weights[c, col] / f32(255), what
                assert want[0][c, col] == 255 or want[1][c] < np.finfo(f32).tiny
    got = run_device(context, queue, weights, pad)
    assert_same(want[1], got[1], f"weights_channel {what}")
    assert_same(want[0], got[0], f"weights8 {what}")
    return want


def test_data_covers_the_cases():
    """The generated weights do contain what the tests are meant to exercise."""
    from katsdpsigproc_amd.rfi import host

    weights, columns = make_weights(1, 8, 257)
    assert sorted(set(ROW_KINDS)) == ["denormal", "inf", "mix", "ties", "zero"]
    assert np.isnan(weights).any() and np.isposinf(weights).any() and np.isneginf(weights).any()
    assert (weights < 0).any() and 0.03 < np.mean(weights[0] == 0) < 0.2
    tiny = np.finfo(f32).tiny
    assert ((weights[0] > 0) & (weights[0] < tiny)).any()
    assert np.all(weights[3] < tiny) and (weights[3] > 0).sum() > 200  # the all-denormal row
    assert not weights[5].any() and np.all(weights[6] == np.inf)
    assert (columns[[5, 6]] == -1).all() and (np.delete(columns, [5, 6]) >= 0).all()
    for c, col in enumerate(columns):
        if col >= 0:
            others = np.delete(weights[c], col)
            ok = (others > 0) & (others < np.inf)
            assert np.all(others[ok] <= weights[c, col] / 2)
    weights8, wc = host.CompressWeightsHost()(weights)
    # the row of ties: scale 2^e, and a tie under every byte but the maximum's
    assert wc[1] == weights[1, columns[1]] / f32(255) and np.log2(float(wc[1])) % 1 == 0
    t = np.delete(weights[1], columns[1]) / wc[1]
    assert np.all((t % 1 == 0.5) | (t == 0)) and np.count_nonzero(t) > 200
    assert weights8[1, columns[1]] == 255 and np.all((weights8[1] % 2 == 0) | (weights8[1] == 255))
    assert wc[5] == 0 and wc[6] == 0 and np.all(weights8[6] == 255) and not weights8[5].any()
    places = {place(k, 37, np.random.RandomState(0)) for k in range(N_PLACES - 1)}
    assert places == {0, 36, 31, 32}
    t = ties_rows(3, 4, 300)
    weights8, wc = host.CompressWeightsHost()(t)
    q = t / wc[:, np.newaxis]
    assert np.count_nonzero(q % 1 == 0.5) == 4 * 299
    assert np.all(weights8[q % 1 == 0.5] % 2 == 0)  # to even: k + 0.5 -> k or k + 1


@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(channels, context, command_queue):
    """Every width; a call with fewer than five rows is repeated with the kinds of its rows
    and the places of their maxima rotated on, so that every place occurs at every shape."""
    for i, baselines in enumerate(BASELINES):
        rotations = range(0, 8, channels) if channels < N_PLACES else [i]
        for rotation in rotations:
            weights, columns = make_weights(channels * 10007 + baselines, channels, baselines,
                                            rotation)  # fmt: skip
            compare(context, command_queue, weights,
                    f"{channels}x{baselines} rotation {rotation}", columns)  # fmt: skip


@pytest.mark.parametrize("channels, baselines", [(3, 70000), (70000, 3), (2, RESIDENT_MAX),
                                                 (2, RESIDENT_MAX + 1)])  # fmt: skip
def test_long_and_tall(channels, baselines, context, command_queue):
    """Rows beyond the register-resident limit, and more rows than a grid dimension of 65535
    could number."""
    weights, columns = make_weights(baselines, channels, baselines)
    assert weights.shape == (channels, baselines)
    compare(context, command_queue, weights, f"{channels}x{baselines}", columns)


@pytest.mark.parametrize("baselines", [65, WAVE_MAX + 1, MEDIUM_MAX + 1, RESIDENT_MAX + 1])
def test_ties(baselines, context, command_queue):
    compare(context, command_queue, ties_rows(baselines, 5, baselines), f"ties 5x{baselines}")


@pytest.mark.parametrize("channels, baselines, pad", [
    (8, 65, 29), (7, 1025, 3), (5, 256, 16), (3, SMALL_MAX + 1, 35), (2, RESIDENT_MAX - 15, 40),
    (2, RESIDENT_MAX + 17, 5)])  # fmt: skip
def test_padding(channels, baselines, pad, context, command_queue):
    """Rows padded beyond what the slots ask for: 2^127 and NaN in the padding of `weights`,
    the sentinel in the padding of `weights8` (run_device looks at it)."""
    weights, columns = make_weights(pad, channels, baselines)
    compare(context, command_queue, weights, f"pad {pad}", columns, pad=pad)


def odd_strides(baselines):
    return (baselines + 6) | 1, (baselines + 2) | 1


def aligned_strides(baselines):
    return -(-baselines // 4) * 4 + 4, -(-baselines // 16) * 16 + 16


@pytest.mark.parametrize("channels, baselines", [(6, 37), (3, SMALL_MAX + 3), (2, RESIDENT_MAX + 232),
                                                 (3, 1), (3, 15), (3, 16), (3, 17), (3, 33)])  # fmt: skip
@pytest.mark.parametrize("offset, strides", [(1, odd_strides), (4, odd_strides), (12, odd_strides),
                                             (16, aligned_strides), (4, aligned_strides)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, channels, baselines, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and a stride of its own per
    array. Odd strides take the element-wise path; 16 elements and strides that keep the rows
    on 16 bytes take the 16-byte path from the middle of an allocation; 4 elements with such
    strides leave `weights` on 16 bytes and `weights8` off them: 16-byte loads, single stores."""
    check_raw_abi(offset, strides, channels, baselines, context, command_queue)


def check_raw_abi(offset, strides, channels, baselines, context, command_queue, views=None):
    """`views` makes the strided arrays (tests/subviews.py: CompactViews unless given) and may
    choose other strides of the same kind."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = views or CompactViews(context, queue)
    weights, columns = make_weights(offset + baselines, channels, baselines, offset)
    weights_stride, weights8_stride = strides(baselines)
    # the rows with their padding as data of the view: 2^127 and NaN, NaN all around it
    padded = hostile_padding((channels, weights_stride))
    padded[:, :baselines] = weights
    d_in = views("weights", f32, padded, weights_stride, offset, poison=True)
    d_out = views("weights8", np.uint8, sentinel_array((channels, baselines), np.uint8),
                  weights8_stride, offset)  # fmt: skip
    d_wc = flat_device_array(context, queue, f32, sentinel_array((1, channels), f32), channels,
                             offset)  # fmt: skip
    _lib.call("ksp_compress_weights", context.device.index, ctypes.c_void_p(queue.stream),
              d_in[1], d_out[1], d_wc[1], channels, baselines, d_in[0].stride, d_out[0].stride)
    want = host.CompressWeightsHost()(weights)
    assert_same(want[1], d_wc[0].read("weights_channel")[0], f"weights_channel at {offset}")
    assert_same(want[0], d_out[0].read("weights8"), f"weights8 at {offset}")
    d_in[0].read("weights")  # (asserts that nothing wrote to it)
    for c, col in enumerate(columns):
        if col >= 0:
            assert want[1][c] == weights[c, col] / f32(255)


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import host, ingest

    template = ingest.CompressWeightsTemplate(context)
    adapter = ingest.CompressWeightsHostFromDevice(template, command_queue)
    for channels, baselines in [(12, 70), (1, 1), (3, SMALL_MAX + 5)]:
        weights, _ = make_weights(11, channels, baselines)
        got = adapter(weights)
        want = host.CompressWeightsHost()(weights)
        assert_same(want[0], got[0], "weights8")
        assert_same(want[1], got[1], "weights_channel")


N_AUTO = 6
LOST = -(2**31)


def chain_dump(seed, channels, in_baselines):
    """Integer noise of amplitude about 1e5 with spikes of 5e6 to 7e6, autocorrelations around
    1e6 in the first N_AUTO baselines, and about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    noise = inputs.generate_data(channels, in_baselines, seed=seed)
    vis = inputs.add_rfi(noise, seed=seed + 100)
    vis_in = np.empty((channels, in_baselines, 2), np.int32)
    vis_in[..., 0] = np.rint(vis.real * 1e5)
    vis_in[..., 1] = np.rint(vis.imag * 1e5)
    vis_in[rs.random_sample((channels, in_baselines)) < 0.03, 0] = LOST
    vis_in[:, :N_AUTO, 0] = 1000000 + np.rint(noise.real[:, :N_AUTO] * 1e5)  # (no spikes, none lost)
    vis_in[:, :N_AUTO, 1] = 0
    return vis_in


def test_behind_the_chain(context, command_queue):
    """Three dumps through prepare -> fused flagger -> accumulate -> finalise -> compress in one
    sequence, against PrepareHost + FlaggerHost + AveragerHost + CompressWeightsHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, in_baselines, cf = 64, 40, 50, 4
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
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, use_weights=True, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    compress = ingest.CompressWeightsTemplate(context).instantiate(queue, channels // cf, baselines)
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "out_weights": ["finalise:weights", "compress:weights"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("compress", compress)], compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("weights") is compress.buffer("weights")
    for name in acc:
        seq.buffer(name).zero(queue)
    rs = np.random.RandomState(9)
    source = rs.permutation(in_baselines)[:baselines].astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    mask = inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * np.uint8(0x20)
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("prepare:channel_flags").set(queue, mask)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    compress_host = host.CompressWeightsHost()

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, mask, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        weights8, weights_channel = compress_host(weights)
        for name, w in (("finalise:vis", vis), ("out_weights", weights), ("finalise:flags", flags),
                        ("compress:weights8", weights8),
                        ("compress:weights_channel", weights_channel)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return weights, weights8, weights_channel

    for d in range(3):
        vis_in = chain_dump(20 + d, channels, in_baselines)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        host_dump(vis_in)
    finalise()
    compress()
    weights, weights8, weights_channel = check_outputs()
    # weights of order 1 per dump: every row has a scale, every sample a byte, and what the
    # consumer expands is the weight to half a step (a whole one where the byte was held up)
    assert np.all(weights_channel > 0) and np.all(weights8 > 0) and np.all(weights8.max(axis=1) == 255)
    assert len(np.unique(weights8)) > 20
    back = compress_host.expand(weights8, weights_channel)
    step = weights_channel[:, np.newaxis]
    assert np.all(np.abs(back - weights) <= np.where(weights8 > 1, step * f32(0.5001), step))
    # and once more through the sequence as a whole
    vis_in = chain_dump(40, channels, in_baselines)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    check_outputs()
