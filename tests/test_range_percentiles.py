"""Range percentiles without a GPU: ``rfi.host.RangePercentilesHost`` against a loop through
``numpy.percentile``, known answers and special values, argument errors, slot wiring and every
launch argument on the fake backend, the sequence finalise -> range percentiles, the argument
checks of ``ksp_range_percentiles`` (which come before any device call), and what the
generators of the GPU tests contain."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_range_percentiles as rp
from tests.fakes import FakeContext

f32 = np.float32
c64 = np.complex64
TINY = rp.TINY
INF = f32(np.inf)


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
    assert len(want) == len(got) == 3
    for name, w, g in zip(("percentiles", "counts", "range_flags"), want, got):
        same_bits(w, g, f"{name} {what}")


# ----------------------------------------------------------- against numpy.percentile
LENGTHS = sorted(set(range(41)) | {63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                                   16383, 16384})  # fmt: skip


@pytest.mark.parametrize("dtype", [f32, c64])
def test_host_against_numpy_percentile(dtype):
    """Every range length, with and without flags, four masks, on values with many ties."""
    start = 3
    for i in range(0, len(LENGTHS), 16):
        lengths = LENGTHS[i : i + 16]
        ranges = [(start, start + n) for n in lengths]
        baselines = start + max(lengths) + 2
        data = rp.make_data(i + 1, 2, baselines, dtype, distinct=29)
        flags = rp.make_flags(i + 2, data.shape)
        for mask in (0, 0x01, 0xFF, 0x28):
            got = host.RangePercentilesHost(ranges, mask)(data, flags)
            same_outputs(rp.loop_reference(data, flags, ranges, mask), got, f"mask {mask}")
            assert got[0].shape == (len(ranges), 5, 2) and got[0].dtype == f32
            assert got[1].shape == (len(ranges), 2) and got[1].dtype == np.uint32
            assert got[2].shape == (len(ranges), 2) and got[2].dtype == np.uint8
        got = host.RangePercentilesHost(ranges)(data)
        assert got[2] is None
        same_outputs(rp.loop_reference(data, None, ranges, 0), got, "no flags")


# ------------------------------------------------------------------------ known answers
def test_known_answers():
    data = np.array([[9, 1, 5, 3, 7, 2, 8, 4, 6],
                     [0.5, 0.5, 2, 2, 2, 1, 1, 1, 1]], f32)  # fmt: skip
    flags = np.array([[0, 2, 0, 1, 0, 0x21, 0x20, 0, 4],
                      [1, 1, 0, 0, 0, 0x41, 0x11, 3, 0x81]], np.uint8)  # fmt: skip
    ranges = [(0, 5), (4, 4), (5, 9)]
    pct, counts, range_flags = host.RangePercentilesHost(ranges, mask=0x01)(data, flags)
    # channel 0: (0, 5) keeps 9 1 5 7 -> sorted 1 5 7 9, indices 0 3 0 2 1; (5, 9) keeps 8 4 6
    # channel 1: (0, 5) keeps 2 2 2; (5, 9) is fully flagged under the mask
    assert pct[0, :, 0].tolist() == [1, 9, 1, 7, 5]
    assert pct[2, :, 0].tolist() == [4, 8, 4, 6, 6]
    assert pct[0, :, 1].tolist() == [2, 2, 2, 2, 2]
    assert pct[1].tolist() == [[0, 0]] * 5 and pct[2, :, 1].tolist() == [0] * 5
    assert not np.signbit(pct).any()
    assert counts.tolist() == [[4, 3], [0, 0], [3, 0]]
    assert range_flags.tolist() == [[3, 1], [0, 0], [0x25, 0xD3]]
    # nothing left out: numpy's own "lower" percentiles of every column range
    pct, counts, range_flags = host.RangePercentilesHost(ranges)(data)
    assert range_flags is None and counts.tolist() == [[5, 5], [0, 0], [4, 4]]
    assert pct[0, :, 0].tolist() == [1, 9, 3, 7, 5]  # 1 3 5 7 9
    assert pct[2, :, 0].tolist() == [2, 8, 2, 6, 4]  # 2 4 6 8: indices 0 3 0 2 1
    assert pct[0, :, 1].tolist() == [0.5, 2, 0.5, 2, 2]


# ----------------------------------------------------------------------- special values
def test_special_values_float():
    nan = np.nan
    data = np.array([[nan, 3, INF, 1, nan, 2], [nan, nan, nan, nan, nan, nan],
                     [0, TINY, 0, 2 * TINY, nan, 0]], f32)  # fmt: skip
    pct, counts, _ = host.RangePercentilesHost([(0, 6), (0, 1), (4, 6)])(data)
    assert counts.tolist() == [[4, 0, 5], [0, 0, 1], [1, 0, 1]]
    assert pct[0, :, 0].tolist() == [1, INF, 1, 3, 2]  # 1 2 3 inf: indices 0 3 0 2 1
    assert pct[:, :, 1].tolist() == [[0] * 5] * 3 and not np.signbit(pct[:, :, 1]).any()
    same_bits(pct[0, :, 2], np.array([0, 2 * TINY, 0, TINY, 0], f32))
    assert pct[2, :, 0].tolist() == [2] * 5 and pct[1, :, 0].tolist() == [0] * 5


def test_special_values_complex():
    specials = rp.COMPLEX_SPECIALS
    data = np.array([[z for z, _ in specials]], c64)
    with np.errstate(all="ignore"):
        amplitude = np.abs(data[0])
    for (z, want), got in zip(specials, amplitude):
        assert (np.isnan(want) and np.isnan(got)) or f32(want) == got, z
    pct, counts, _ = host.RangePercentilesHost([(0, len(specials)), (0, 2), (2, 4)])(data)
    assert counts[:, 0].tolist() == [len(specials) - 2, 0, 2]  # (nan, 1), (1, nan) are left out
    assert pct[1, :, 0].tolist() == [0] * 5
    assert pct[2, :, 0].tolist() == [INF] * 5  # (inf, nan) and (3e38, 3e38): both +inf, kept
    # 0, tiny, 3 tiny, inf, inf, inf: indices 0 5 1 3 2
    same_bits(pct[0, :, 0], np.array([0, INF, TINY, INF, 3 * TINY], f32))
    same_outputs(rp.loop_reference(data, None, [(0, 8), (0, 2), (2, 4)], 0),
                 host.RangePercentilesHost([(0, 8), (0, 2), (2, 4)])(data))  # fmt: skip


# ------------------------------------------------------------------------------- errors
BAD_RANGES = [[], [(0, 1)] * 17, [(2, 1)], [(-1, 3)], [(0, 16385)], [(0, 1, 2)], [(0.0, 1)],
              [(0, True)], 5, [3]]  # fmt: skip


def test_host_errors():
    for bad in BAD_RANGES:
        with pytest.raises(ValueError, match="ranges"):
            host.RangePercentilesHost(bad)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            host.RangePercentilesHost([(0, 1)], mask=bad)
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match="mask"):
            host.RangePercentilesHost([(0, 1)], mask=bad)
    assert host.RangePercentilesHost([[0, 16384], (np.int32(5), np.int64(5))]).ranges == (
        (0, 16384), (5, 5))  # fmt: skip
    fn = host.RangePercentilesHost([(0, 4), (2, 6)], mask=1)
    data, flags = np.ones((3, 6), f32), np.zeros((3, 6), np.uint8)
    fn(data, flags)
    fn(data.astype(c64), flags)
    for bad in (data.astype(np.float64), data.astype(np.complex128), data.astype(np.int32),
                data[0], data[np.newaxis], np.zeros((0, 6), f32), np.zeros((3, 0), f32)):  # fmt: skip
        with pytest.raises(ValueError, match="data"):
            fn(bad, flags)
    for bad in (flags.astype(np.int8), flags.astype(bool), flags[:2], flags[:, :5], flags[0]):
        with pytest.raises(ValueError, match="flags"):
            fn(data, bad)
    with pytest.raises(ValueError, match="ranges"):
        fn(data[:, :5], flags[:, :5])  # (2, 6) ends beyond 5 baselines
    with pytest.raises(TypeError, match="mask"):
        fn(data)
    assert host.RangePercentilesHost([(0, 4)])(data)[2] is None


def test_template_and_operation_errors(context, queue):
    Template = ingest.RangePercentilesTemplate
    with pytest.raises(ValueError):
        Template(context, tuning={"wgs": 256})
    assert Template(context, tuning={}).tuning == {}
    assert Template.autotune(context) == {}
    assert Template.host_class is host.RangePercentilesHost
    assert Template.KERNEL == "ksp_range_percentiles"
    assert Template(context).kernel.name == "ksp_range_percentiles"
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            Template(context, mask=bad)
    with pytest.raises(TypeError, match="mask"):
        Template(context, mask=1.0)
    with pytest.raises(ValueError, match="mask"):
        Template(context, use_flags=False, mask=1)
    template = Template(context, mask=0xFF)
    assert (template.is_amplitude, template.use_flags, template.mask) == (False, True, 0xFF)
    for args in [(0, 4), (4, 0), (-4, 4), (4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args, [(0, 0)])
    for bad in BAD_RANGES + [[(0, 7)], [(7, 7)]]:
        with pytest.raises(ValueError, match="ranges"):
            template.instantiate(queue, 4, 6, bad)
    fn = template.instantiate(queue, 4, 6, [(6, 6), (0, 6)])
    assert isinstance(fn, ingest.RangePercentiles) and fn.ranges == ((6, 6), (0, 6))


def test_host_from_device(context, queue):
    ranges = [(0, 3), (1, 5)]
    with pytest.raises(ValueError, match="ranges"):
        ingest.RangePercentilesHostFromDevice(ingest.RangePercentilesTemplate(context), queue, [])
    with_flags = ingest.RangePercentilesHostFromDevice(
        ingest.RangePercentilesTemplate(context, mask=1), queue, ranges)  # fmt: skip
    without = ingest.RangePercentilesHostFromDevice(
        ingest.RangePercentilesTemplate(context, is_amplitude=True, use_flags=False), queue, ranges)  # fmt: skip
    data, flags = np.ones((4, 5), c64), np.zeros((4, 5), np.uint8)
    with pytest.raises(TypeError, match="flags"):
        with_flags(data)
    with pytest.raises(TypeError, match="flags"):
        without(data.real.copy(), flags)
    for bad in (np.ones(5, c64), np.ones((2, 3, 4), c64), np.ones((0, 5), c64)):
        with pytest.raises(ValueError):
            with_flags(bad, flags)
    with pytest.raises(ValueError, match="ranges"):
        with_flags(data[:, :4], flags[:, :4])
    assert not queue.launches
    pct, counts, range_flags = with_flags(data, flags)
    assert (pct.shape, pct.dtype) == ((2, 5, 4), f32)
    assert (counts.shape, counts.dtype) == ((2, 4), np.uint32)
    assert (range_flags.shape, range_flags.dtype) == ((2, 4), np.uint8)
    pct, counts, range_flags = without(np.ones((4, 5), f32))
    assert range_flags is None and pct.shape == (2, 5, 4) and counts.shape == (2, 4)
    assert [name for name, _ in queue.launches] == ["ksp_range_percentiles"] * 2


# ------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("is_amplitude", [False, True])
@pytest.mark.parametrize("use_flags", [False, True])
def test_wiring(is_amplitude, use_flags, context, queue):
    mask = 0x28 if use_flags else 0
    template = ingest.RangePercentilesTemplate(context, is_amplitude, use_flags, mask)
    ranges = [(10, 200), (0, 0), (3, 4)]
    fn = template.instantiate(queue, 300, 200, ranges)
    shapes = {"data": (300, 200), "percentiles": (3, 5, 300), "counts": (3, 300)}
    dtypes = {"data": f32 if is_amplitude else c64, "percentiles": f32, "counts": np.uint32}
    if use_flags:
        shapes.update(flags=(300, 200), range_flags=(3, 300))
        dtypes.update(flags=np.uint8, range_flags=np.uint8)
    assert set(fn.slots) == set(shapes)
    for name, shape in shapes.items():
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes[name]
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len(dims) == (11 if use_flags else 7) and len({id(d) for d in dims}) == len(dims)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["data"].dimensions[1])
    accel.Dimension(300, min_padded_size=333).link(fn.slots["counts"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_range_percentiles"]  # one launch
    args = queue.launches[0][1]
    assert len(args) == 16
    assert args[0] is fn.buffer("data").buffer
    assert args[2] is fn.buffer("percentiles").buffer
    assert args[3] is fn.buffer("counts").buffer
    if use_flags:
        assert args[1] is fn.buffer("flags").buffer
        assert args[4] is fn.buffer("range_flags").buffer
    else:
        assert args[1] is None and args[4] is None
    assert all(isinstance(a, np.int32) for a in args[5:12] + args[13:])
    assert [int(a) for a in args[5:7]] == [300, 200]
    data_stride = 512  # 500 rounded up to whole 128-byte rows, for either type
    assert fn.buffer("data").padded_shape == (300, data_stride)
    assert fn.buffer("percentiles").padded_shape == (3, 5, 320)
    counts_stride = fn.buffer("counts").padded_shape[1]
    assert counts_stride >= 333 and fn.buffer("counts").padded_shape[0] == 3
    want = [data_stride, 0, 320, counts_stride, 0]
    if use_flags:
        want[1] = fn.buffer("flags").padded_shape[1]
        want[4] = fn.buffer("range_flags").padded_shape[1]
        assert want[1] == 256 and want[4] == 384
    assert [int(a) for a in args[7:12]] == want
    assert isinstance(args[12], ctypes.Array) and args[12]._type_ is ctypes.c_int
    assert list(args[12]) == [10, 200, 0, 0, 3, 4]
    assert [int(a) for a in args[13:]] == [3, int(is_amplitude), mask]
    assert fn.parameters() == {
        "is_amplitude": is_amplitude, "use_flags": use_flags, "mask": mask,
        "ranges": [[10, 200], [0, 0], [3, 4]], "channels": 300, "baselines": 200}  # fmt: skip
    fn()
    assert len(queue.launches) == 2


def test_behind_finalise(context, queue):
    """finalise -> range percentiles: `vis` and `flags` are one buffer each, one padded size."""
    channels, baselines, cf = 256, 200, 4
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    ranges = [(0, 20), (20, 200)]
    percentiles = ingest.RangePercentilesTemplate(context, mask=0xFF).instantiate(
        queue, channels // cf, baselines, ranges)  # fmt: skip
    # more row padding than either asks for, asked of the other member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["vis"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=700).link(percentiles.slots["flags"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("percentiles", percentiles)],
        compounds={"vis": ["finalise:vis", "percentiles:data"],
                   "flags": ["finalise:flags", "percentiles:flags"]})  # fmt: skip
    for name in ("finalise:vis", "percentiles:data", "finalise:flags", "percentiles:flags"):
        assert name not in seq.slots
    assert {"vis", "flags", "finalise:weights", "percentiles:percentiles", "percentiles:counts",
            "percentiles:range_flags"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_average_finalise", "ksp_range_percentiles"]
    final_args, args = (launch[1] for launch in queue.launches)
    assert finalise.buffer("vis") is percentiles.buffer("data") is seq.buffer("vis")
    assert finalise.buffer("flags") is percentiles.buffer("flags") is seq.buffer("flags")
    assert final_args[3] is args[0] is seq.buffer("vis").buffer
    assert final_args[5] is args[1] is seq.buffer("flags").buffer
    vis_stride, flags_stride = seq.buffer("vis").padded_shape[1], seq.buffer("flags").padded_shape[1]
    assert (vis_stride, flags_stride) == (304, 768)  # whole 128-byte rows
    assert int(final_args[13]) == int(args[7]) == vis_stride
    assert int(final_args[15]) == int(args[8]) == flags_stride
    assert [int(a) for a in args[5:7]] == [channels // cf, baselines]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first

    def call(data=p, flags=p, percentiles=p, counts=p, range_flags=p, channels=4, baselines=8,
             in_stride=8, flags_stride=8, out_stride=4, counts_stride=4, range_flags_stride=4,
             ranges=(0, 8, 2, 2), n_ranges=None, is_amplitude=0, mask=1, ok=False):  # fmt: skip
        if n_ranges is None:
            n_ranges = len(ranges) // 2
        array = (ctypes.c_int * len(ranges))(*ranges) if ranges is not None else None
        rc = lib.ksp_range_percentiles(0, None, data, flags, percentiles, counts, range_flags,
                                       channels, baselines, in_stride, flags_stride, out_stride,
                                       counts_stride, range_flags_stride, array, n_ranges,
                                       is_amplitude, mask)  # fmt: skip
        if ok:
            assert rc == 0, _lib.last_error()
            return ""
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: in is NULL" in call(data=None)
    assert "invalid argument: percentiles is NULL" in call(percentiles=None)
    assert "invalid argument: counts is NULL" in call(counts=None)
    assert "invalid argument: ranges is NULL" in call(ranges=None, n_ranges=1)
    both = "invalid argument: flags and range_flags must both be NULL or both be given"
    assert both in call(flags=None)
    assert both in call(range_flags=None)
    assert "invalid argument: mask must be 0 without flags" in call(flags=None, range_flags=None)
    for bad in (-1, 256):
        assert "invalid argument: mask must be 0..255" in call(mask=bad)
    assert "invalid argument: channels must not be negative" in call(channels=-1)
    for bad in (0, -1):
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    assert "invalid argument: n_ranges must be 1..16" in call(n_ranges=0)
    assert "invalid argument: n_ranges must be 1..16" in call(ranges=(0, 1) * 17)
    assert "invalid argument: in_stride is smaller than baselines" in call(in_stride=7)
    assert "invalid argument: flags_stride is smaller than baselines" in call(flags_stride=7)
    assert "invalid argument: out_stride is smaller than channels" in call(out_stride=3)
    assert "invalid argument: counts_stride is smaller than channels" in call(counts_stride=3)
    assert "invalid argument: range_flags_stride is smaller than channels" in call(
        range_flags_stride=3)  # fmt: skip
    # the order of the checks: everything wrong at once, then only every stride
    strides = dict(in_stride=-1, flags_stride=-1, out_stride=-1, counts_stride=-1,
                   range_flags_stride=-1)  # fmt: skip
    assert "invalid argument: in is NULL" in call(
        data=None, flags=None, percentiles=None, counts=None, range_flags=None, channels=-1,
        baselines=0, ranges=None, n_ranges=0, mask=-1, **strides)  # fmt: skip
    assert "invalid argument: in_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: out_stride is smaller than channels" in call(
        **dict(strides, in_stride=8, flags_stride=8))  # fmt: skip
    inside = "invalid argument: a range must satisfy 0 <= start <= stop <= baselines"
    for bad in [(-1, 4), (5, 4), (0, 9), (9, 9)]:
        assert inside in call(ranges=(0, 8) + bad)
    assert "invalid argument: a range is longer than 16384 columns" in call(
        baselines=20000, in_stride=20000, flags_stride=20000, ranges=(3, 16388))  # fmt: skip
    assert inside in call(baselines=20000, in_stride=20000, flags_stride=20000, ranges=(3, 20001))
    # without flags their strides are ignored; no channels is no work and no device call
    call(channels=0, out_stride=0, counts_stride=0, range_flags_stride=0, ok=True)
    call(channels=0, flags=None, range_flags=None, mask=0, flags_stride=0, out_stride=0,
         counts_stride=0, range_flags_stride=-1, ranges=(0, 8) * 16, ok=True)  # fmt: skip


# ------------------------------------------------------- the inputs of the GPU tests
def test_data_covers_the_cases():
    tiny = np.finfo(f32).tiny
    for dtype in (f32, c64):
        data = rp.make_data(5, 5, 4097, dtype)
        with np.errstate(all="ignore"):
            a = np.abs(data) if dtype == c64 else data
        assert a.dtype == f32 and not np.signbit(a).any()
        assert np.isnan(a).sum() > 50 and np.isposinf(a).sum() > 50 and (a == 0).sum() > 50
        assert ((a > 0) & (a < tiny)).sum() > 50
        values, repeats = np.unique(a[0][np.isfinite(a[0])], return_counts=True)
        assert (repeats > 20).sum() > 30 and len(values) > 800  # ties, and free values
        if dtype == c64:
            assert len(np.unique(data[0])) > 3 * 37  # the same amplitude from different samples
            for z, _ in rp.COMPLEX_SPECIALS:
                same = (data.real == z.real) | (np.isnan(data.real) & np.isnan(z.real))
                same &= (data.imag == z.imag) | (np.isnan(data.imag) & np.isnan(z.imag))
                assert same.any(), z
        assert not np.isnan(rp.make_data(5, 3, 500, dtype, special=0.0)).any()
    flags = rp.make_flags(3, (8, 4000))
    assert 0.2 < np.mean(flags & 1 != 0) < 0.3
    assert set(np.unique(flags)) >= {0, 1, 8, 0x20, 0x80, 0x29}
    for length in (9, 65, 1025, 4097):
        data, flags, ranges, kept = rp.kept_count_case(length, length, c64)
        assert kept == [0, 1, 2, 3, 4, 5, 8, length - 1, length]
        (start, stop), = ranges
        assert start % 2 == 1 and stop - start == length and stop < data.shape[1]
        counts = host.RangePercentilesHost(ranges, 0x01)(data, flags)[1]
        assert counts[0].tolist() == kept
        assert not (flags[:, :start] & 1).any() and not (flags[:, stop:] & 1).any()
    ranges = rp.LAYOUT_RANGES
    assert len(ranges) == 16 and len(set(ranges)) == 15  # one repeated
    lengths = [stop - start for start, stop in ranges]
    assert lengths[0] == 0 and lengths[-1] == 0 and 0 in lengths[1:-1] and 1 in lengths
    assert (0, rp.LAYOUT_BASELINES) in ranges
    assert sum(start % 2 for start, _ in ranges) >= 6
    assert any(a < c and d < b for a, b in ranges for c, d in ranges)  # nested
    assert any(a < c < b < d for a, b in ranges for c, d in ranges)  # overlapping
    assert [s for s, _ in ranges] != sorted(s for s, _ in ranges)
    host.check_ranges(ranges, rp.LAYOUT_BASELINES)
