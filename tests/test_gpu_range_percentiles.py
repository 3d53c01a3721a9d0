"""Range percentiles on the GPU (``rfi.ingest.RangePercentilesTemplate``,
``ksp_range_percentiles``): every comparison is of bit patterns, against
``rfi.host.RangePercentilesHost``, over every element of every output."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests import inputs_range_percentiles as rp
from tests.subviews import SENTINEL, CompactViews, sentinel_array

pytestmark = pytest.mark.gpu

# The range lengths at which csrc/range_percentiles.hip changes path: up to WAVE_MAX a wavefront
# per (channel, range) with 4 keys per lane, then the workgroup with 8 keys per lane up to
# T8_MAX, 16 up to T16_MAX, 32 up to T32_MAX and 64 up to MAX_LENGTH, the longest range.
WAVE_MAX = 256
T8_MAX = 2048
T16_MAX = 4096
T32_MAX = 8192
MAX_LENGTH = 16384
PATH_LIMITS = [WAVE_MAX, T8_MAX, T16_MAX, T32_MAX]
LENGTHS = sorted(
    set(range(10)) | {15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                      MAX_LENGTH - 1, MAX_LENGTH}
    | {limit + d for limit in PATH_LIMITS for d in (-1, 0, 1)})  # fmt: skip
STARTS = [0, 1, 3, 4]
CHANNELS = [1, 2, 5]
f32 = np.float32
c64 = np.complex64
HUGE = rp.HUGE  # finite: a kernel that reads it has a wrong maximum (NaN would be left out)
NAMES = ("percentiles", "counts", "range_flags")


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
    assert len(want) == len(got) == 3
    for name, w, g in zip(NAMES, want, got):
        assert_same(w, g, f"{name} {what}")


def hostile(shape, dtype):
    """What paddings and unused columns hold: 2^127 and 0 in turn (0xFF and 0 for flags)."""
    raw = np.zeros(shape, dtype)
    raw.reshape(-1)[0::2] = 0xFF if np.dtype(dtype) == np.uint8 else HUGE
    return raw


def run_device(context, queue, data, flags, ranges, mask=0, pad=0):
    """The outputs of the operation. The paddings of `data` and `flags` are hostile, the outputs
    start out full of sentinel bytes and their paddings are checked afterwards."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    channels, baselines = data.shape
    template = ingest.RangePercentilesTemplate(context, data.dtype == f32, flags is not None, mask)
    fn = template.instantiate(queue, channels, baselines, ranges)
    outputs = ["percentiles", "counts"] + (["range_flags"] if flags is not None else [])
    if pad:
        for name in ["data"] + (["flags"] if flags is not None else []) + outputs:
            dim = fn.slots[name].dimensions[-1]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    for name, value in (("data", data), ("flags", flags)):
        if value is not None:
            buffer = fn.buffer(name)
            assert buffer.padded_shape[1] >= baselines + pad
            raw = hostile(buffer.padded_shape, value.dtype)
            raw[:, :baselines] = value
            queue.enqueue_write_buffer(buffer.buffer, raw)
    for name in outputs:
        buffer = fn.buffer(name)
        assert buffer.padded_shape[-1] >= channels + pad
        assert buffer.padded_shape[:-1] == buffer.shape[:-1]
        queue.enqueue_write_buffer(buffer.buffer, sentinel_array(buffer.padded_shape, buffer.dtype))
    fn()
    result = []
    for name in outputs:
        buffer = fn.buffer(name)
        raw = np.empty(buffer.padded_shape, buffer.dtype)
        queue.enqueue_read_buffer(buffer.buffer, raw)
        assert np.all(raw[..., channels:].view(np.uint8) == SENTINEL), f"wrote into the padding of {name}"
        result.append(np.ascontiguousarray(raw[..., :channels]))
    return result + [None] * (3 - len(result))


def compare(context, queue, data, flags, ranges, mask, what, pad=0):
    from katsdpsigproc_amd.rfi import host

    want = host.RangePercentilesHost(ranges, mask)(data, flags)
    assert_outputs(want, run_device(context, queue, data, flags, ranges, mask, pad), what)
    return want


# --------------------------------------------------------------------------- length sweep
@pytest.mark.parametrize("mask", [0, 0x01])
@pytest.mark.parametrize("dtype", [f32, c64])
def test_lengths(dtype, mask, context, command_queue):
    """Every length from every start for 1, 2 and 5 channels, up to 16 ranges per call."""
    whole = rp.make_data(int(mask) + 10, max(CHANNELS), STARTS[-1] + MAX_LENGTH + 2, dtype)
    whole_flags = rp.make_flags(int(mask) + 20, whole.shape)
    kept_some = set()
    for channels in CHANNELS:
        for start in STARTS:
            for i in range(0, len(LENGTHS), 16):
                lengths = LENGTHS[i : i + 16]
                ranges = [(start, start + n) for n in lengths]
                baselines = start + max(lengths) + 2
                data = np.ascontiguousarray(whole[:channels, :baselines])
                flags = np.ascontiguousarray(whole_flags[:channels, :baselines]) if mask else None
                want = compare(context, command_queue, data, flags, ranges, mask,
                               f"{channels} channels, start {start}, lengths {lengths}")  # fmt: skip
                for n, count in zip(lengths, want[1]):
                    if np.any((count > 0) & (count < n)):
                        kept_some.add(n)
    assert kept_some >= {n for n in LENGTHS if n >= 255}  # samples were left out, not all


# ------------------------------------------------------------------------ kept-count sweep
@pytest.mark.parametrize("length", [9, 65, 1025, 4097])
@pytest.mark.parametrize("dtype", [f32, c64])
def test_kept_counts(dtype, length, context, command_queue):
    """Rows with exactly 0, 1, 2, 3, 4, 5, 8, n - 1 and n samples kept."""
    data, flags, ranges, kept = rp.kept_count_case(length, length, dtype)
    want = compare(context, command_queue, data, flags, ranges, 0x01, f"length {length}")
    assert want[1][0].tolist() == kept


# ------------------------------------------------------------------ ties and special values
def special_rows(dtype, baselines):
    """Rows of three distinct values, one value, zeros, denormals, +inf, NaN, and everything."""
    rs = np.random.RandomState(baselines)
    few = np.array([0.75, 3.0, 1e-3], f32)[rs.randint(3, size=baselines)]
    rows = [few, np.full(baselines, 2.5, f32), np.zeros(baselines, f32),
            (rs.randint(1, 50, baselines) * np.float64(rp.TINY)).astype(f32),
            np.full(baselines, np.inf, f32), np.full(baselines, np.nan, f32)]  # fmt: skip
    mixed = few.copy()
    what = rs.random_sample(baselines)
    for i, value in enumerate(rp.FLOAT_SPECIALS):
        mixed[(what >= 0.1 * i) & (what < 0.1 * i + 0.1)] = value
    amplitudes = np.array(rows + [mixed], f32)
    if np.dtype(dtype) == f32:
        return amplitudes
    # the same amplitudes as real, negative real, imaginary and negative imaginary numbers
    turn = np.array([1, -1, 1j, -1j], c64)[rs.randint(4, size=amplitudes.shape)]
    with np.errstate(all="ignore"):
        data = np.where(np.isfinite(amplitudes), amplitudes * turn, amplitudes + 0j).astype(c64)
    data[5, 0::2] = complex(1, np.nan)  # (the all-NaN row: NaN in either part)
    pairs = np.array([z for z, _ in rp.COMPLEX_SPECIALS], c64)
    return np.vstack([data, pairs[rs.randint(len(pairs), size=baselines)][np.newaxis]])


@pytest.mark.parametrize("dtype", [f32, c64])
def test_ties_and_special_values(dtype, context, command_queue):
    baselines = 4100
    data = special_rows(dtype, baselines)
    ranges = [(0, baselines), (1, 66), (3, 1028), (2, 2), (3, 4100), (0, 7), (2049, 4098)]
    flags = rp.make_flags(9, data.shape)
    want = compare(context, command_queue, data, None, ranges, 0, "without flags")
    assert np.all(want[1][:, 5] == 0) and not want[0][:, :, 5].any()  # the NaN row
    assert np.all(want[0][0, :, 4] == np.inf) and np.all(want[0][0, :, 1] == 2.5)
    assert np.all(want[0][0, :, 2] == 0) and want[1][0, 2] == baselines
    compare(context, command_queue, data, flags, ranges, 0x01, "mask 0x01")
    compare(context, command_queue, data, flags, ranges, 0xFF, "mask 0xFF")


# ---------------------------------------------------------------------------- range layout
@pytest.mark.parametrize("dtype", [f32, c64])
def test_range_layout(dtype, context, command_queue):
    """16 ranges in one call, and single ranges."""
    data = rp.make_data(31, 3, rp.LAYOUT_BASELINES, dtype)
    flags = rp.make_flags(32, data.shape)
    compare(context, command_queue, data, flags, rp.LAYOUT_RANGES, 0x01, "16 ranges")
    compare(context, command_queue, data, None, rp.LAYOUT_RANGES[::-1], 0, "16 ranges reversed")
    for single in [(1235, 4996), (7, 7), (4999, 5000)]:
        compare(context, command_queue, data, flags, [single], 0x08, f"one range {single}")


# --------------------------------------------------------------------------------- padding
@pytest.mark.parametrize("dtype", [f32, c64])
@pytest.mark.parametrize("channels, pad", [(5, 29), (2, 3), (7, 16)])
def test_padding_and_outside_the_ranges(channels, pad, dtype, context, command_queue):
    """Columns outside every range hold 2^127 and 0 in turn (flags 0xFF and 0), as the row
    paddings do; every slot is padded beyond what it asks for."""
    baselines = 4700
    ranges = [(5, 70), (70, 70), (333, 1358), (1358, 1423), (2001, 4500)]
    inside = np.zeros(baselines, bool)
    for start, stop in ranges:
        inside[start:stop] = True
    assert not inside[:5].any() and not inside[4500:].any() and not inside[1423:2001].any()
    data = hostile((channels, baselines), dtype)
    flags = hostile((channels, baselines), np.uint8)
    data[:, inside] = rp.make_data(pad, channels, baselines, dtype)[:, inside]
    flags[:, inside] = rp.make_flags(pad + 1, (channels, baselines))[:, inside]
    want = compare(context, command_queue, data, flags, ranges, 0x01, f"pad {pad}", pad=pad)
    assert not np.any(want[0] == HUGE)
    compare(context, command_queue, data, None, ranges, 0, f"pad {pad}, no flags", pad=pad)


# ------------------------------------------------------------------------------- sub-views
def odd_strides(baselines, channels):
    return [(baselines + 6) | 1, (baselines + 2) | 1, (channels + 4) | 1, (channels + 8) | 1,
            (channels + 12) | 1]  # fmt: skip


def aligned_strides(baselines, channels):
    return [-(-baselines // 16) * 16 + 16 * k for k in (1, 2)] + [
        -(-channels // 16) * 16 + 16 * k for k in (1, 2, 3)]  # fmt: skip


@pytest.mark.parametrize("dtype", [f32, c64])
@pytest.mark.parametrize("use_flags", [True, False])
@pytest.mark.parametrize("offset, strides", [(1, odd_strides), (4, odd_strides), (12, odd_strides),
                                             (16, aligned_strides), (4, aligned_strides),
                                             (1, aligned_strides)])  # fmt: skip
def test_raw_abi_subviews(offset, strides, use_flags, dtype, context, command_queue):
    """Pointers `offset` elements into their allocations and a stride of its own per array:
    odd strides take the element-wise path in most rows, 16 elements with strides that keep the
    rows on 16 bytes take the 16-byte loads where a range starts on one."""
    check_raw_abi(offset, strides, use_flags, dtype, context, command_queue)


def check_raw_abi(offset, strides, use_flags, dtype, context, command_queue, views=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind: the launcher gets the strides of the views."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = views or CompactViews(context, queue)
    channels, baselines = 6, 2500
    ranges = [(0, 64), (64, 321), (4, 2400), (321, 321), (7, 2500), (2436, 2500)]
    mask = 0x01 if use_flags else 0
    stride = dict(zip(("data", "flags") + NAMES, strides(baselines, channels)))
    # the rows with their padding as data of the view, poison all around it
    padded = hostile((channels, stride["data"]), dtype)
    padded[:, :baselines] = rp.make_data(offset, channels, baselines, dtype)
    padded_flags = hostile((channels, stride["flags"]), np.uint8)
    padded_flags[:, :baselines] = rp.make_flags(offset + 1, (channels, baselines))

    def make(name, dtype, data, poison=False):
        made = views(name, dtype, data, stride[name], offset, poison)
        stride[name] = made[0].stride
        return made

    d_data = make("data", dtype, padded, poison=True)
    d_flags = make("flags", np.uint8, padded_flags, poison=True)
    n = len(ranges)
    shapes = {"percentiles": (5 * n, channels), "counts": (n, channels), "range_flags": (n, channels)}
    dtypes = {"percentiles": f32, "counts": np.uint32, "range_flags": np.uint8}
    out = {name: make(name, dtypes[name], sentinel_array(shapes[name], dtypes[name]))
           for name in NAMES}  # fmt: skip
    null = ctypes.c_void_p(0)
    _lib.call("ksp_range_percentiles", context.device.index, ctypes.c_void_p(queue.stream),
              d_data[1], d_flags[1] if use_flags else null, out["percentiles"][1],
              out["counts"][1], out["range_flags"][1] if use_flags else null, channels, baselines,
              stride["data"], stride["flags"], stride["percentiles"], stride["counts"],
              stride["range_flags"], (ctypes.c_int * (2 * n))(*[v for r in ranges for v in r]), n,
              int(np.dtype(dtype) == f32), mask)  # fmt: skip
    data = np.ascontiguousarray(padded[:, :baselines])
    flags = np.ascontiguousarray(padded_flags[:, :baselines]) if use_flags else None
    want = host.RangePercentilesHost(ranges, mask)(data, flags)
    assert_same(want[0].reshape(5 * n, channels), out["percentiles"][0].read("percentiles"),
                f"percentiles at {offset}")  # fmt: skip
    assert_same(want[1], out["counts"][0].read("counts"), f"counts at {offset}")
    got_flags = out["range_flags"][0].read("range_flags")
    if use_flags:
        assert_same(want[2], got_flags, f"range_flags at {offset}")
    else:
        assert np.all(got_flags == SENTINEL)  # not an output of this call: untouched
    d_data[0].read("data")  # (asserts that nothing wrote to it)
    d_flags[0].read("flags")


# ------------------------------------------------------------------------------------ tall
def test_tall(context, command_queue):
    """More rows than a grid dimension of 65535 could number."""
    channels, baselines = 70000, 8
    data = np.tile(rp.make_data(70, 1000, baselines, c64), (70, 1))
    flags = np.tile(rp.make_flags(71, (700, baselines)), (100, 1))
    data[-1] = 3 + 4j
    flags[-1] = 0
    assert data.shape == flags.shape == (channels, baselines)
    want = compare(context, command_queue, data, flags, [(0, 8), (3, 8), (2, 2)], 0x01, "tall")
    assert want[0][0, 1, -1] == 5


# ------------------------------------------------------------------ parity with Percentile5
@pytest.mark.parametrize("dtype", [f32, c64])
def test_parity_with_percentile5(dtype, context, command_queue):
    from katsdpsigproc_amd import percentile

    queue = command_queue
    shape = (6, 8320)
    ranges = [(0, 64), (64, 1064), (2272, 4288), (3000, 8000)]
    data = rp.make_data(16, *shape, dtype, special=0.0)
    assert not np.isnan(data).any()
    got = run_device(context, queue, data, None, ranges)
    template = percentile.Percentile5Template(context, 8320, is_amplitude=np.dtype(dtype) == f32)
    for r, column_range in enumerate(ranges):
        fn = template.instantiate(queue, shape, column_range)
        fn.ensure_all_bound()
        fn.buffer("src").set(queue, data)
        fn()
        assert_same(fn.buffer("dest").get(queue), got[0][r], f"Percentile5 of {column_range}")
        assert np.all(got[1][r] == column_range[1] - column_range[0])


# --------------------------------------------------------------------------------- adapter
@pytest.mark.parametrize("use_flags", [True, False])
def test_host_from_device(use_flags, context, command_queue):
    from katsdpsigproc_amd.rfi import host, ingest

    mask = 0x28 if use_flags else 0
    for dtype, (channels, baselines) in [(c64, (12, 70)), (f32, (1, 1)), (c64, (3, T16_MAX + 5))]:
        ranges = [(0, baselines), (baselines // 2, baselines), (0, 0), (0, 1)]
        template = ingest.RangePercentilesTemplate(context, dtype == f32, use_flags, mask)
        adapter = ingest.RangePercentilesHostFromDevice(template, command_queue, ranges)
        data = rp.make_data(17, channels, baselines, dtype)
        flags = rp.make_flags(18, data.shape) if use_flags else None
        assert_outputs(host.RangePercentilesHost(ranges, mask)(data, flags), adapter(data, flags),
                       f"{channels} x {baselines}")  # fmt: skip


# ------------------------------------------------------------------------ behind the chain
def test_behind_the_chain(context, command_queue):
    """Two dumps through fused flagger -> accumulate -> finalise -> range percentiles in one
    sequence, against FlaggerHost + AveragerHost + RangePercentilesHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, cf = 64, 40, 4
    ranges = [(0, 6), (6, 40), (0, 40), (40, 40)]
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
    percentiles = ingest.RangePercentilesTemplate(context, mask=0xFF).instantiate(
        queue, channels // cf, baselines, ranges)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["flagger:vis", "accumulate:vis"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "input_flags": ["flagger:input_flags", "accumulate:input_flags"],
        "out_vis": ["finalise:vis", "percentiles:data"],
        "out_flags": ["finalise:flags", "percentiles:flags"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("flagger", flagger), ("accumulate", accumulate), ("finalise", finalise),
                ("percentiles", percentiles)], compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert finalise.buffer("vis") is percentiles.buffer("data")
    assert finalise.buffer("flags") is percentiles.buffer("flags")
    for name in acc:
        seq.buffer(name).zero(queue)
    # samples without data in every dump: whole output channels of a few baselines
    input_flags = np.zeros((channels, baselines), np.uint8)
    for out_channel, baseline in [(2, 1), (5, 7), (5, 8), (9, 30), (9, 3)]:
        input_flags[out_channel * cf : (out_channel + 1) * cf, baseline] = 0x20
    seq.buffer("input_flags").set(queue, input_flags)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    percentiles_host = host.RangePercentilesHost(ranges, 0xFF)

    def host_dump(vis):
        averager.add(vis, flagger_host(vis, input_flags), input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        want = percentiles_host(vis, flags)
        for name, w in (("out_vis", vis), ("finalise:weights", weights), ("out_flags", flags),
                        ("percentiles:percentiles", want[0]), ("percentiles:counts", want[1]),
                        ("percentiles:range_flags", want[2])):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return want

    for d in range(2):
        vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=50 + d), seed=60 + d)
        seq.buffer("vis").set(queue, vis)
        flagger()
        accumulate()
        host_dump(vis)
    finalise()
    percentiles()
    _, counts, range_flags = check_outputs()
    lengths = np.array([stop - start for start, stop in ranges])[:, np.newaxis]
    assert np.any((counts > 0) & (counts < lengths))  # the exclusion is exercised
    assert 0 < counts[0, 2] <= 5 and 0 < counts[1, 5] <= 32 and range_flags[0, 2] & 0x20
    assert not counts[3].any() and not range_flags[3].any()
    # and once more through the sequence as a whole
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=70), seed=71)
    seq.buffer("vis").set(queue, vis)
    seq()
    host_dump(vis)
    check_outputs()
