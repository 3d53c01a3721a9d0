"""Band averages on the GPU (``rfi.ingest.BandAverageTemplate``, ``ksp_band_average``): every
comparison is of bit patterns, against ``rfi.host.BandAverageHost``, over every element of
every output."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests import inputs_band_average as ba
from tests.subviews import SENTINEL, CompactViews, flat_device_array, sentinel_array

pytestmark = pytest.mark.gpu

# csrc/band_average.hip: blocks of 128 channels, walked in chunks of 8, 4 or 2 rows for up to 2, 4
# or 8 series with the remainder row by row; a wavefront owns 64 baselines, a workgroup 256.
CHANNELS = [1, 2, 127, 128, 129, 255, 256, 257, 1000]
BASELINES = [1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
N_SERIES = [1, 3, 8]
f32 = np.float32
c64 = np.complex64
HUGE = ba.HUGE
NAMES = ba.NAMES


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def assert_same(want, got, what=""):
    if want is None or got is None:
        assert want is None and got is None, what
        return
    assert want.dtype == got.dtype and want.shape == got.shape, what
    bits = np.uint8 if want.dtype.itemsize == 1 else np.uint32  # (complex64: two words)
    want = np.ascontiguousarray(want).view(bits)
    got = np.ascontiguousarray(got).view(bits)
    bad = want != got
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} elements differ, first at "
        f"{np.argwhere(bad)[0]}: want {want[bad][0]:#010x}, got {got[bad][0]:#010x}")  # fmt: skip


def assert_outputs(want, got, what=""):
    assert len(want) == len(got) == 5
    for name, w, g in zip(NAMES, want, got):
        assert_same(w, g, f"{name} {what}")


def hostile(shape, dtype):
    """What paddings hold: 2^127 (in both parts) and 0 in turn, 0xFF and 0 for flags."""
    raw = np.zeros(shape, dtype)
    raw.reshape(-1)[0::2] = {np.dtype(np.uint8): 0xFF, np.dtype(c64): complex(HUGE, HUGE)}.get(
        np.dtype(dtype), HUGE)  # fmt: skip
    return raw


def run_device(context, queue, data, weights, flags, mask=0, pad=0):
    """The outputs of the operation. The paddings of the inputs are hostile, the work area and
    the outputs start out full of sentinel bytes and the outputs' paddings are checked."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    channels, baselines = data.shape
    template = ingest.BandAverageTemplate(context, flags is not None, mask)
    fn = template.instantiate(queue, channels, baselines, weights.shape[0])
    given = {"data": data, "channel_weights": weights, "flags": flags}
    outputs = [name for name in NAMES if name != "series_flags" or flags is not None]
    if pad:
        for name in [name for name, value in given.items() if value is not None] + outputs:
            dim = fn.slots[name].dimensions[-1]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    for name, value in given.items():
        if value is not None:
            buffer = fn.buffer(name)
            assert buffer.padded_shape[1] >= value.shape[1] + pad
            raw = hostile(buffer.padded_shape, value.dtype)
            raw[:, : value.shape[1]] = value
            queue.enqueue_write_buffer(buffer.buffer, raw)
    for name in outputs + ["work_area"]:
        buffer = fn.buffer(name)
        assert buffer.padded_shape[:-1] == buffer.shape[:-1]
        queue.enqueue_write_buffer(buffer.buffer, sentinel_array(buffer.padded_shape, buffer.dtype))
    fn()
    result = []
    for name in outputs:
        buffer = fn.buffer(name)
        assert buffer.padded_shape[-1] >= baselines + pad
        raw = np.empty(buffer.padded_shape, buffer.dtype)
        queue.enqueue_read_buffer(buffer.buffer, raw)
        assert np.all(raw[..., baselines:].view(np.uint8) == SENTINEL), f"wrote into the padding of {name}"
        result.append(np.ascontiguousarray(raw[..., :baselines]))
    return result + [None] * (5 - len(result))


def compare(context, queue, data, weights, flags, mask, what, pad=0):
    from katsdpsigproc_amd.rfi import host

    want = host.BandAverageHost(mask)(data, weights, flags)
    assert_outputs(want, run_device(context, queue, data, weights, flags, mask, pad), what)
    return want


# ------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("use_flags", [True, False])
def test_sizes(use_flags, context, command_queue):
    """A third of channels x baselines, every value of either with every series count."""
    seen_c, seen_b = set(), set()
    for ci, channels in enumerate(CHANNELS):
        for bi, baselines in enumerate(BASELINES):
            if (ci + bi) % 3 != 0:
                continue
            n_series = N_SERIES[(bi // 3 + ci) % 3]
            seen_c.add((channels, n_series))
            seen_b.add(baselines)
            data = ba.make_data(ci * 100 + bi, channels, baselines)
            weights = ba.make_weights(ci * 100 + bi + 50, n_series, channels)
            flags = ba.make_flags(ci * 100 + bi + 70, data.shape) if use_flags else None
            want = compare(context, command_queue, data, weights, flags, ba.MASK * use_flags,
                           f"{channels} x {baselines}, {n_series} series")  # fmt: skip
            if use_flags and channels >= 127:
                assert np.all((want[3] > 0) & (want[3] < channels))  # some left out, not all
    assert seen_b == set(BASELINES)
    assert seen_c == {(c, n) for c in CHANNELS for n in N_SERIES}


# ------------------------------------------------------------------------- long, narrow, wide
@pytest.mark.parametrize("channels, baselines, n_series", [(70000, 3, 3), (262144, 2, 1),
                                                           (3, 70000, 3)])  # fmt: skip
def test_long_and_wide(channels, baselines, n_series, context, command_queue):
    """More blocks than fit the unrolled combining loop many times over, the longest band, and
    more baselines than one grid row of 65535 workgroups of single lanes would hold."""
    data = ba.make_data(channels, channels, baselines)
    weights = ba.make_weights(channels + 1, n_series, channels)
    flags = ba.make_flags(channels + 2, data.shape)
    want = compare(context, command_queue, data, weights, flags, ba.MASK,
                   f"{channels} x {baselines}")  # fmt: skip
    assert want[3].max() > channels // 3
    compare(context, command_queue, data, weights, None, 0, f"{channels} x {baselines}, no flags")


# --------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("channels, baselines, pad", [(130, 257, 29), (5, 100, 3), (300, 64, 16)])
def test_padding(channels, baselines, pad, context, command_queue):
    """Every slot padded beyond what it asks for; 2^127 and 0xFF in the paddings of the inputs,
    sentinels in the outputs and their paddings."""
    data = ba.make_data(pad, channels, baselines)
    weights = ba.make_weights(pad + 1, 3, channels)
    flags = ba.make_flags(pad + 2, data.shape)
    want = compare(context, command_queue, data, weights, flags, ba.MASK, f"pad {pad}", pad=pad)
    assert np.all(np.abs(want[0]) < 2.0**22) and not np.any(want[4] == 0xFF)
    compare(context, command_queue, data, weights, None, 0, f"pad {pad}, no flags", pad=pad)


# ------------------------------------------------------------------------------- sub-views
STRIDE_NAMES = ("data", "flags", "channel_weights") + NAMES


def odd_strides(baselines, channels):
    return [(baselines + 6) | 1, (baselines + 2) | 1, (channels + 4) | 1] + [
        (baselines + 4 * k) | 1 for k in range(2, 7)]  # fmt: skip


def aligned_strides(baselines, channels):
    up = -(-baselines // 16) * 16
    return [up + 16, up + 32, channels + 3] + [up + 16 * k for k in range(3, 8)]


@pytest.mark.parametrize("use_flags", [True, False])
@pytest.mark.parametrize("offset, strides", [(1, odd_strides), (4, odd_strides), (12, odd_strides),
                                             (16, aligned_strides), (2, aligned_strides),
                                             (1, aligned_strides)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, use_flags, context, command_queue):
    """Pointers `offset` elements into their allocations and a stride of its own per array, odd
    ones and ones that keep the rows on 16 bytes: samples are loaded one by one either way."""
    check_raw_abi(offset, strides, use_flags, context, command_queue)


def check_raw_abi(offset, strides, use_flags, context, command_queue, views=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind: the launcher gets the strides of the views."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = views or CompactViews(context, queue)
    channels, baselines, n_series = 260, 333, 3
    mask = ba.MASK if use_flags else 0
    stride = dict(zip(STRIDE_NAMES, strides(baselines, channels)))
    # the rows with their padding as data of the view, poison all around it
    padded = hostile((channels, stride["data"]), c64)
    padded[:, :baselines] = ba.make_data(offset, channels, baselines)
    padded_flags = hostile((channels, stride["flags"]), np.uint8)
    padded_flags[:, :baselines] = ba.make_flags(offset + 1, (channels, baselines))
    padded_weights = hostile((n_series, stride["channel_weights"]), f32)
    padded_weights[:, :channels] = ba.make_weights(offset + 2, n_series, channels)

    def make(name, dtype, data, poison=False):
        made = views(name, dtype, data, stride[name], offset, poison)
        stride[name] = made[0].stride
        return made

    d_data = make("data", c64, padded, poison=True)
    d_flags = make("flags", np.uint8, padded_flags, poison=True)
    d_weights = make("channel_weights", f32, padded_weights, poison=True)
    dtypes = dict(zip(NAMES, (c64, f32, f32, np.uint32, np.uint8)))
    out = {name: make(name, dtypes[name], sentinel_array((n_series, baselines), dtypes[name]))
           for name in NAMES}  # fmt: skip
    work_bytes = _lib.load().ksp_band_average_work_bytes(channels, baselines, n_series)
    assert work_bytes == 3 * n_series * 5 * baselines * 4
    # the work area at an offset too, with a margin that has to survive
    d_work = flat_device_array(context, queue, f32, sentinel_array((1, work_bytes // 4), f32),
                               work_bytes // 4, offset)  # fmt: skip
    null = ctypes.c_void_p(0)
    _lib.call("ksp_band_average", context.device.index, ctypes.c_void_p(queue.stream),
              d_data[1], d_flags[1] if use_flags else null, d_weights[1], out["mean"][1],
              out["mean_amplitude"][1], out["weight_sums"][1], out["counts"][1],
              out["series_flags"][1] if use_flags else null, d_work[1], work_bytes, channels,
              baselines, n_series, *[stride[name] for name in STRIDE_NAMES], mask)  # fmt: skip
    data = np.ascontiguousarray(padded[:, :baselines])
    flags = np.ascontiguousarray(padded_flags[:, :baselines]) if use_flags else None
    weights = np.ascontiguousarray(padded_weights[:, :channels])
    want = host.BandAverageHost(mask)(data, weights, flags)
    for name, w in zip(NAMES[:4], want):
        assert_same(w, out[name][0].read(name), f"{name} at {offset}")
    got_flags = out["series_flags"][0].read("series_flags")
    if use_flags:
        assert_same(want[4], got_flags, f"series_flags at {offset}")
    else:
        assert np.all(got_flags == SENTINEL)  # not an output of this call: untouched
    d_work[0].read("work_area")  # (asserts that nothing around it was written)
    for view, name in ((d_data, "data"), (d_flags, "flags"), (d_weights, "channel_weights")):
        view[0].read(name)  # (asserts that nothing wrote to it)


# -------------------------------------------------------------------------- special values
def test_special_values(context, command_queue):
    data, weights, flags, mask = ba.special_case()
    want = compare(context, command_queue, data, weights, flags, mask, "special values")
    assert want[0][2, 2].real == np.inf and not want[3][:, 3].any() and not want[3][1].any()
    assert 0 < want[2][3, 0] < np.finfo(f32).tiny  # a denormal weight sum
    compare(context, command_queue, data, weights, flags, 0xFF, "special values, every bit")
    compare(context, command_queue, data, weights, None, 0, "special values, no flags")


# ------------------------------------------------------------------------ series that overlap
def test_overlapping_and_identical_series(context, command_queue):
    channels, baselines = 300, 70
    data = ba.make_data(21, channels, baselines)
    flags = ba.make_flags(22, data.shape)
    one = ba.make_weights(23, 1, channels)
    want = compare(context, command_queue, data, np.repeat(one, 8, axis=0), flags, ba.MASK,
                   "eight equal series")  # fmt: skip
    for value in want:
        assert np.all(value.view(np.uint8) == value[:1].view(np.uint8))
    weights = np.zeros((4, channels), f32)
    weights[0, :200] = one[0, :200]  # two overlapping sub-bands, the whole band, one channel
    weights[1, 100:] = one[0, 100:]
    weights[2] = one[0]
    weights[3, 128] = 0.7
    want = compare(context, command_queue, data, weights, flags, ba.MASK, "overlapping series")
    assert set(np.unique(want[3][3])) == {0, 1}


# --------------------------------------------------------------------------------- adapter
@pytest.mark.parametrize("use_flags", [True, False])
def test_host_from_device(use_flags, context, command_queue):
    from katsdpsigproc_amd.rfi import host, ingest

    mask = 0x21 if use_flags else 0
    template = ingest.BandAverageTemplate(context, use_flags, mask)
    adapter = ingest.BandAverageHostFromDevice(template, command_queue)
    for channels, baselines, n_series in [(12, 70, 2), (1, 1, 1), (200, 5, 8)]:
        data = ba.make_data(17, channels, baselines)
        weights = ba.make_weights(18, n_series, channels)
        flags = ba.make_flags(19, data.shape) if use_flags else None
        assert_outputs(host.BandAverageHost(mask)(data, weights, flags),
                       adapter(data, weights, flags), f"{channels} x {baselines}")  # fmt: skip


# ------------------------------------------------------------------------ behind the chain
def test_behind_the_chain(context, command_queue):
    """Two dumps through fused flagger -> accumulate -> finalise -> band average in one
    sequence, against FlaggerHost + AveragerHost + BandAverageHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, cf, n_series = 64, 40, 4, 3
    full = device.BackgroundFlags.FULL
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=full),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, use_weights=False, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    average = ingest.BandAverageTemplate(context, mask=0xFF).instantiate(
        queue, channels // cf, baselines, n_series)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["flagger:vis", "accumulate:vis"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "input_flags": ["flagger:input_flags", "accumulate:input_flags"],
        "out_vis": ["finalise:vis", "average:data"],
        "out_flags": ["finalise:flags", "average:flags"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("flagger", flagger), ("accumulate", accumulate), ("finalise", finalise),
                ("average", average)], compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is average.buffer("data")
    assert finalise.buffer("flags") is average.buffer("flags")
    for name in acc:
        seq.buffer(name).zero(queue)
    # samples without data in every dump: whole output channels of a few baselines
    input_flags = np.zeros((channels, baselines), np.uint8)
    for out_channel, baseline in [(2, 1), (5, 7), (5, 8), (9, 30), (9, 3)]:
        input_flags[out_channel * cf : (out_channel + 1) * cf, baseline] = 0x20
    seq.buffer("input_flags").set(queue, input_flags)
    weights = ba.make_weights(40, n_series, channels // cf)
    weights[0, 2] = weights[0, 5] = 0.37  # series 0 takes the channels without data
    weights[1, 2] = 0
    seq.buffer("average:channel_weights").set(queue, weights)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    average_host = host.BandAverageHost(0xFF)

    def host_dump(vis):
        averager.add(vis, flagger_host(vis, input_flags), input_flags=input_flags)

    def check_outputs():
        vis, out_weights, flags = averager.finalise()
        want = average_host(vis, weights, flags)
        for name, w in [("out_vis", vis), ("finalise:weights", out_weights), ("out_flags", flags)] + [
                ("average:" + name, w) for name, w in zip(NAMES, want)]:  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return want

    for d in range(2):
        vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=50 + d), seed=60 + d)
        seq.buffer("vis").set(queue, vis)
        flagger()
        accumulate()
        host_dump(vis)
    finalise()
    average()
    _, _, _, counts, series_flags = check_outputs()
    in_0 = int((weights[0] > 0).sum())
    assert 0 < counts[0, 1] < in_0 and 0 < counts[0, 7] < in_0  # the exclusion is exercised
    assert series_flags[0, 1] & 0x20 and not series_flags[1, 1] & 0x20
    assert np.any(counts[0] == in_0)
    # and once more through the sequence as a whole
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=70), seed=71)
    seq.buffer("vis").set(queue, vis)
    seq()
    host_dump(vis)
    check_outputs()
