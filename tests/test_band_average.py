"""Band averages without a GPU: ``rfi.host.BandAverageHost`` against known answers, a triple
loop of ``np.float32`` scalars and float64, special values, argument errors, slot wiring and
every launch argument on the fake backend, the sequence finalise -> band average, and the
argument checks of ``ksp_band_average`` (which come before any device call)."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_band_average as ba
from tests.fakes import FakeContext

f32 = np.float32
c64 = np.complex64
BLOCK = host.BandAverageHost.BLOCK


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def same_bits(want, got, what=""):
    if want is None or got is None:
        assert want is None and got is None, what
        return
    assert want.dtype == got.dtype and want.shape == got.shape, what
    np.testing.assert_array_equal(np.ascontiguousarray(want).view(np.uint8),
                                  np.ascontiguousarray(got).view(np.uint8), what)  # fmt: skip


def same_outputs(want, got, what=""):
    assert len(want) == len(got) == 5
    for name, w, g in zip(ba.NAMES, want, got):
        same_bits(w, g, f"{name} {what}")


# ------------------------------------------------------------------------ known answers
def test_known_answers():
    nan = np.nan
    data = np.array([[1, 3 + 4j], [2j, complex(nan, 0)], [6 + 8j, 1 + 1j]], c64)
    weights = np.array([[1, 1, 0], [0.5, 0, 0.25]], f32)
    flags = np.array([[0, 0], [4, 0], [0, 1]], np.uint8)
    mean, amplitude, sums, counts, series_flags = host.BandAverageHost(mask=1)(data, weights, flags)
    same_bits(mean, np.array([[0.5 + 1j, 3 + 4j],
                              [complex(f32(2) / f32(0.75), f32(2) / f32(0.75)), 3 + 4j]], c64))  # fmt: skip
    assert f32(2) / f32(0.75) == f32(2.6666667)
    same_bits(amplitude, np.array([[1.5, 5], [4, 5]], f32))
    same_bits(sums, np.array([[2, 1], [0.75, 0.5]], f32))
    same_bits(counts, np.array([[2, 1], [2, 1]], np.uint32))
    same_bits(series_flags, np.array([[4, 0], [0, 1]], np.uint8))
    assert host.BandAverageHost.BLOCK == 128 and host.BandAverageHost.MAX_SERIES == 8


# ------------------------------------------------------------------ against the scalar loop
@pytest.mark.parametrize("channels", [1, 127, 128, 129, 300])
def test_host_against_scalar_loop(channels):
    data = ba.make_data(channels, channels, 7)
    weights = ba.make_weights(channels + 1, 3, channels)
    flags = ba.make_flags(channels + 2, data.shape)
    assert channels < 100 or 0.2 < np.mean(weights == 0) < 0.4
    assert channels < 100 or 0.2 < np.mean(flags & ba.MASK != 0) < 0.4
    assert channels < 100 or np.any(flags & ba.OTHER_BIT)
    for mask in (ba.MASK, 0, 0xFF):
        got = host.BandAverageHost(mask)(data, weights, flags)
        same_outputs(ba.loop_reference(data, weights, flags, mask), got, f"mask {mask}")
        for value, dtype in zip(got, (c64, f32, f32, np.uint32, np.uint8)):
            assert value.shape == (3, 7) and value.dtype == dtype
    got = host.BandAverageHost()(data, weights)
    assert got[4] is None
    same_outputs(ba.loop_reference(data, weights, None, 0), got, "no flags")


# ------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("channels", [1, 127, 128, 129, 300, 4096])
def test_mean_amplitude_against_float64(channels):
    """The first-order bound of the blocked sum, the multiply and the division, once for the
    numerator and once for the denominator; all terms are positive."""
    data = ba.make_data(channels + 10, channels, 7)
    weights = ba.make_weights(channels + 11, 3, channels)
    flags = ba.make_flags(channels + 12, data.shape)
    _, amplitude, _, counts, _ = host.BandAverageHost(ba.MASK)(data, weights, flags)
    n_blocks = -(-channels // BLOCK)
    bound = 2 * (min(channels, BLOCK) + n_blocks + 4) * 2.0**-24
    a64 = np.abs(data.astype(np.complex128))
    kept = (flags & ba.MASK) == 0
    worst = 0.0
    for k in range(3):
        w = np.where(weights[k] > 0, weights[k], 0).astype(np.float64)[:, np.newaxis] * kept
        want = (w * a64).sum(axis=0) / np.where(counts[k] > 0, w.sum(axis=0), 1)
        some = counts[k] > 0
        assert np.array_equal(some, (w > 0).any(axis=0))
        error = np.abs(amplitude[k][some] - want[some]) / want[some]
        worst = max(worst, error.max() / bound) if some.any() else worst
        assert np.all(error <= bound), f"{error.max()} > {bound}"
    print(f"channels {channels}: worst error {worst:.3f} of the bound")


# ----------------------------------------------------------------------- special values
def test_special_values():
    data, weights, flags, mask = ba.special_case()
    got = host.BandAverageHost(mask)(data, weights, flags)
    same_outputs(ba.loop_reference(data, weights, flags, mask), got)
    mean, amplitude, sums, counts, series_flags = got
    channels = data.shape[0]
    in_0 = weights[0] > 0
    # a NaN real part and a NaN imaginary part: left out, not counted
    assert counts[2, 1] == channels - 4 and counts[2, 0] == channels
    assert counts[0, 1] == in_0.sum() - in_0[[3, 130, 4, 299]].sum()
    assert np.isfinite(mean[:, 1]).all() and np.isfinite(amplitude[:, 1]).all()
    # +inf: kept and propagated
    assert counts[2, 2] == channels and mean[2, 2].real == np.inf and amplitude[2, 2] == np.inf
    assert mean[2, 2].imag == f32(sum_in_blocks(data[:, 2].imag)) / f32(channels)
    # a series without a usable weight: zeros, count 0, flags 0
    for value in got:
        assert not value[1].view(np.uint8).any()
    # everything flagged: zeros, count 0, series_flags set
    assert not counts[[0, 2, 3], 3].any() and not sums[:, 3].any() and not mean[:, 3].any()
    assert not amplitude[:, 3].any() and series_flags[[0, 2, 3], 3].tolist() == [0x21] * 3
    # all NaN: the same, with the flags of a bit outside the mask
    assert not counts[:, 4].any() and not mean[:, 4].any() and series_flags[2, 4] == 0x80
    # flagged samples in channels of weight 0 do not reach the series
    assert series_flags[0, 5] == 0 and counts[0, 5] == in_0.sum()
    assert series_flags[2, 5] == 0x41 and counts[2, 5] == in_0.sum()
    # denormal products: not flushed
    tiny = np.finfo(f32).tiny
    assert 0 < sums[3, 0] < tiny and sums[3, 0] == f32(channels) * f32(2.0**-140)
    assert 0 < amplitude[2, 6] < tiny and counts[3, 6] == channels
    assert np.abs(mean[3, 0] - mean[2, 0]) < 0.02  # the quotient of two denormal sums
    for value in (mean, amplitude):  # zeros and negative zeros: +0.0
        assert not np.ascontiguousarray(value[[0, 2, 3], 7]).view(np.uint32).any()
    assert not np.isnan(mean).any() and not np.isnan(amplitude).any()


def sum_in_blocks(values):
    total = f32(0)
    for start in range(0, len(values), BLOCK):
        partial = f32(0)
        for v in values[start : start + BLOCK]:
            partial = f32(partial + v)
        total = f32(total + partial)
    return total


def test_long_band_is_quick():
    """262144 channels through the host: blocks at once, not a loop over channels."""
    channels = 262144
    data = np.ones((channels, 2), c64)
    weights = np.full((1, channels), 0.5, f32)
    mean, amplitude, sums, counts, series_flags = host.BandAverageHost()(data, weights)
    assert series_flags is None and counts.tolist() == [[channels] * 2]
    assert sums.tolist() == [[channels / 2] * 2] and mean.tolist() == [[1, 1]]


def test_order_of_the_sums_shows():
    """The inputs of the GPU tests tell one order of summation from another: the cancelling
    baseline as one running sum, without blocks, differs from the definition, and so does
    every mean of the band taken backwards."""
    data = ba.make_data(5, 1000, 4)
    weights = ba.make_weights(6, 1, 1000, zero=0.0)
    mean = host.BandAverageHost()(data, weights)[0]
    running = f32(0)
    for c in range(1000):
        running = f32(running + f32(weights[0, c] * data[c, -1].real))
    assert f32(running / weights[0].sum(dtype=f32)) != mean[0, -1].real
    backwards = host.BandAverageHost()(data[::-1], weights[:, ::-1])[0]
    assert np.all(backwards.view(np.uint32) != mean.view(np.uint32))


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            host.BandAverageHost(mask=bad)
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match="mask"):
            host.BandAverageHost(mask=bad)
    fn = host.BandAverageHost(mask=1)
    data, flags = np.ones((3, 6), c64), np.zeros((3, 6), np.uint8)
    weights = np.ones((2, 3), f32)
    fn(data, weights, flags)
    for bad in (data.astype(np.complex128), data.real.copy(), data[0], data[np.newaxis],
                np.zeros((0, 6), c64), np.zeros((3, 0), c64)):  # fmt: skip
        with pytest.raises(ValueError, match="data"):
            fn(bad, weights, flags)
    with pytest.raises(ValueError, match="data"):
        fn(np.broadcast_to(c64(1), (262145, 1)), np.broadcast_to(f32(1), (1, 262145)))
    for bad in (weights.astype(np.float64), weights[0], weights[:, :2], np.ones((0, 3), f32),
                np.ones((9, 3), f32), np.ones((3, 2), f32), weights[np.newaxis]):  # fmt: skip
        with pytest.raises(ValueError, match="channel_weights"):
            fn(data, bad, flags)
    for bad in (flags.astype(np.int8), flags.astype(bool), flags[:2], flags[:, :5], flags[0]):
        with pytest.raises(ValueError, match="flags"):
            fn(data, weights, bad)
    with pytest.raises(TypeError, match="mask"):
        fn(data, weights)
    assert host.BandAverageHost()(data, np.ones((8, 3), f32))[4] is None


def test_template_and_operation_errors(context, queue):
    Template = ingest.BandAverageTemplate
    with pytest.raises(ValueError):
        Template(context, tuning={"wgs": 256})
    assert Template(context, tuning={}).tuning == {}
    assert Template.autotune(context) == {}
    assert Template.host_class is host.BandAverageHost
    assert Template.KERNEL == "ksp_band_average"
    assert Template(context).kernel.name == "ksp_band_average"
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            Template(context, mask=bad)
    with pytest.raises(TypeError, match="mask"):
        Template(context, mask=1.0)
    with pytest.raises(ValueError, match="mask"):
        Template(context, use_flags=False, mask=1)
    template = Template(context, mask=0xFF)
    assert (template.use_flags, template.mask) == (True, 0xFF)
    for args in [(0, 4), (4, 0), (-4, 4), (4, -1), (262145, 4), (4, 4, 0), (4, 4, 9), (4, 4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    fn = template.instantiate(queue, 262144, 2)
    assert isinstance(fn, ingest.BandAverage) and fn.n_series == 1
    assert template.instantiate(queue, 1, 1, 8).n_series == 8


def test_host_from_device(context, queue):
    with_flags = ingest.BandAverageHostFromDevice(ingest.BandAverageTemplate(context, mask=1), queue)
    without = ingest.BandAverageHostFromDevice(
        ingest.BandAverageTemplate(context, use_flags=False), queue)  # fmt: skip
    data, flags = np.ones((4, 5), c64), np.zeros((4, 5), np.uint8)
    weights = np.ones((3, 4), f32)
    with pytest.raises(TypeError, match="flags"):
        with_flags(data, weights)
    with pytest.raises(TypeError, match="flags"):
        without(data, weights, flags)
    for bad in (np.ones(5, c64), np.ones((2, 3, 4), c64), np.ones((0, 5), c64)):
        with pytest.raises(ValueError):
            with_flags(bad, weights, flags)
    with pytest.raises(ValueError):
        with_flags(data, np.ones((9, 4), f32), flags)
    assert not queue.launches
    out = with_flags(data, weights, flags)
    for value, dtype in zip(out, (c64, f32, f32, np.uint32, np.uint8)):
        assert (value.shape, value.dtype) == ((3, 5), dtype)
    out = without(data, weights)
    assert out[4] is None and all(value.shape == (3, 5) for value in out[:4])
    assert [name for name, _ in queue.launches] == ["ksp_band_average"] * 2


# ------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("use_flags", [False, True])
def test_wiring(use_flags, context, queue):
    mask = 0x28 if use_flags else 0
    template = ingest.BandAverageTemplate(context, use_flags, mask)
    fn = template.instantiate(queue, 300, 200, 3)
    work_bytes = 3 * 3 * 5 * 200 * 4  # three blocks of 128 channels, three series
    assert ingest.BandAverage.work_bytes(300, 200, 3) == work_bytes
    assert ingest.BandAverage.work_bytes(128, 1, 1) == 20
    assert ingest.BandAverage.work_bytes(129, 1, 8) == 320
    series = ("mean", "mean_amplitude", "weight_sums", "counts")
    shapes = {"data": (300, 200), "channel_weights": (3, 300), "work_area": (work_bytes,)}
    shapes.update({name: (3, 200) for name in series})
    dtypes = {"data": c64, "channel_weights": f32, "mean": c64, "mean_amplitude": f32,
              "weight_sums": f32, "counts": np.uint32, "work_area": np.uint8}  # fmt: skip
    if use_flags:
        shapes.update(flags=(300, 200), series_flags=(3, 200))
        dtypes.update(flags=np.uint8, series_flags=np.uint8)
    assert set(fn.slots) == set(shapes)
    for name, shape in shapes.items():
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes[name]
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len(dims) == (17 if use_flags else 13) and len({id(d) for d in dims}) == len(dims)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["data"].dimensions[1])
    accel.Dimension(200, min_padded_size=333).link(fn.slots["counts"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_band_average"]  # one call
    args = queue.launches[0][1]
    assert len(args) == 22
    order = ["data", "flags", "channel_weights", "mean", "mean_amplitude", "weight_sums",
             "counts", "series_flags", "work_area"]  # fmt: skip
    for arg, name in zip(args, order):
        if name in fn.slots:
            assert arg is fn.buffer(name).buffer, name
        else:
            assert arg is None, name
    assert isinstance(args[9], np.uint64) and int(args[9]) == work_bytes
    assert fn.buffer("work_area").padded_shape == (work_bytes,)
    assert fn.required_bytes() == sum(fn.buffer(name).buffer.nbytes for name in fn.slots)
    assert fn.required_bytes() > work_bytes + 300 * 512 * 8
    assert all(isinstance(a, np.int32) for a in args[10:])
    assert [int(a) for a in args[10:13]] == [300, 200, 3]
    assert fn.buffer("data").padded_shape == (300, 512)  # 500 rounded up to whole 128-byte rows
    strides = [fn.buffer(name).padded_shape[1] if name in fn.slots else 0 for name in order[:8]]
    assert strides[0] == 512 and strides[2] >= 300 and strides[6] >= 333
    assert all(fn.buffer(name).padded_shape[0] == 3 for name in series)
    if use_flags:
        assert strides[1] >= 200 and strides[7] >= 200
    assert [int(a) for a in args[13:21]] == strides
    assert int(args[21]) == mask
    assert fn.parameters() == {"use_flags": use_flags, "mask": mask, "n_series": 3,
                               "channels": 300, "baselines": 200}  # fmt: skip
    fn()
    assert len(queue.launches) == 2


def test_behind_finalise(context, queue):
    """finalise -> band average: `vis` and `flags` are one buffer each, one padded size."""
    channels, baselines, cf = 256, 200, 4
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    average = ingest.BandAverageTemplate(context, mask=0xFF).instantiate(
        queue, channels // cf, baselines, 2)  # fmt: skip
    # more row padding than either asks for, asked of the other member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["vis"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=700).link(average.slots["flags"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("average", average)],
        compounds={"vis": ["finalise:vis", "average:data"],
                   "flags": ["finalise:flags", "average:flags"]})  # fmt: skip
    for name in ("finalise:vis", "average:data", "finalise:flags", "average:flags"):
        assert name not in seq.slots
    assert {"vis", "flags", "finalise:weights", "average:channel_weights", "average:mean",
            "average:mean_amplitude", "average:weight_sums", "average:counts",
            "average:series_flags", "average:work_area"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_average_finalise", "ksp_band_average"]
    final_args, args = (launch[1] for launch in queue.launches)
    assert finalise.buffer("vis") is average.buffer("data") is seq.buffer("vis")
    assert finalise.buffer("flags") is average.buffer("flags") is seq.buffer("flags")
    assert final_args[3] is args[0] is seq.buffer("vis").buffer
    assert final_args[5] is args[1] is seq.buffer("flags").buffer
    vis_stride, flags_stride = seq.buffer("vis").padded_shape[1], seq.buffer("flags").padded_shape[1]
    assert (vis_stride, flags_stride) == (304, 768)  # whole 128-byte rows
    assert int(final_args[13]) == int(args[13]) == vis_stride
    assert int(final_args[15]) == int(args[14]) == flags_stride
    assert [int(a) for a in args[10:13]] == [channels // cf, baselines, 2]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_work_bytes(lib):
    for args in [(1, 1, 1), (128, 7, 3), (129, 7, 3), (300, 200, 8), (262144, 2, 1),
                 (4096, 8320, 8), (262144, 2**31 - 1, 8)]:  # fmt: skip
        assert lib.ksp_band_average_work_bytes(*args) == ingest.BandAverage.work_bytes(*args)
    for args in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1)]:
        assert lib.ksp_band_average_work_bytes(*args) == 0


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first
    names = ["data", "flags", "channel_weights", "mean", "mean_amplitude", "weight_sums",
             "counts", "series_flags", "work_area"]  # fmt: skip

    def call(channels=300, baselines=8, n_series=2, work_bytes=None, mask=1, **kwargs):
        pointers = [kwargs.pop(name, p) for name in names]
        strides = [kwargs.pop(name, channels if name == "channel_weights_stride" else baselines)
                   for name in ("data_stride", "flags_stride", "channel_weights_stride",
                                "mean_stride", "mean_amplitude_stride", "weight_sums_stride",
                                "counts_stride", "series_flags_stride")]  # fmt: skip
        assert not kwargs
        if work_bytes is None:
            work_bytes = 3 * n_series * 5 * baselines * 4
        rc = lib.ksp_band_average(0, None, *pointers, work_bytes, channels, baselines, n_series,
                                  *strides, mask)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in names:
        if name not in ("flags", "series_flags"):
            assert f"invalid argument: {name} is NULL" in call(**{name: None})
    both = "invalid argument: flags and series_flags must both be NULL or both be given"
    assert both in call(flags=None)
    assert both in call(series_flags=None)
    assert "invalid argument: mask must be 0 without flags" in call(flags=None, series_flags=None)
    for bad in (-1, 256):
        assert "invalid argument: mask must be 0..255" in call(mask=bad)
    for bad in (0, -1, 262145):
        assert "invalid argument: channels must be 1..262144" in call(
            channels=bad, channel_weights_stride=300000)  # fmt: skip
    for bad in (0, -1):
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -1, 9):
        assert "invalid argument: n_series must be 1..8" in call(n_series=bad)
    for name in ("data", "flags", "mean", "mean_amplitude", "weight_sums", "counts",
                 "series_flags"):  # fmt: skip
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})  # fmt: skip
    assert "invalid argument: channel_weights_stride is smaller than channels" in call(
        channel_weights_stride=299)  # fmt: skip
    # the order of the checks: everything wrong at once, then only every stride
    strides = {name + "_stride": -1 for name in names[:-1]}
    assert "invalid argument: data is NULL" in call(
        channels=0, baselines=0, n_series=0, work_bytes=0, mask=-1, **dict.fromkeys(names),
        **strides)  # fmt: skip
    assert "invalid argument: data_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: channel_weights_stride is smaller than channels" in call(
        **dict(strides, data_stride=8, flags_stride=8))  # fmt: skip
    assert "invalid argument: work_area is not 4-byte aligned" in call(
        work_area=ctypes.c_void_p(66))  # fmt: skip
    small = "invalid argument: work_area is smaller than ksp_band_average_work_bytes"
    assert small in call(work_bytes=3 * 2 * 5 * 8 * 4 - 1)
    assert small in call(work_bytes=0)
    assert small in call(channels=385, channel_weights_stride=385)  # a fourth block
    # without flags their strides are ignored: the first complaint is about something else
    assert small in call(flags=None, series_flags=None, mask=0, flags_stride=0,
                         series_flags_stride=-1, work_bytes=0)  # fmt: skip
