"""Compressing weights without a GPU: ``rfi.host.CompressWeightsHost`` against known answers
and a double loop of float32 scalars, its properties over random rows, argument errors, slot
wiring and every launch argument on the fake backend, the sequence finalise -> compress, and the
argument checks of ``ksp_compress_weights``, which come before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests.fakes import FakeContext

f32 = np.float32
TINY = f32(2.0**-149)  # the smallest denormal


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def same_bits(want, got):
    assert want.dtype == got.dtype and want.shape == got.shape
    np.testing.assert_array_equal(np.ascontiguousarray(want).view(np.uint8),
                                  np.ascontiguousarray(got).view(np.uint8))  # fmt: skip


def compress(rows):
    weights8, weights_channel = host.CompressWeightsHost()(np.array(rows, f32))
    assert weights8.dtype == np.uint8 and weights_channel.dtype == f32
    assert weights8.shape == np.shape(rows) and weights_channel.shape == (len(rows),)
    return weights8, weights_channel


# ------------------------------------------------------------------------ known answers
def test_known_row():
    weights8, wc = compress([[np.nan, -1, -0.0, 0, np.inf, 1, 2, TINY]])
    # 1 / wc is 127.5 or the float32 below it (127 as a tie to even or from just below, never
    # 128); the denormal is held up to 1
    assert weights8.tolist() == [[0, 0, 0, 0, 255, 127, 255, 1]]
    assert wc[0] == f32(2) / f32(255)
    assert f32(127.49999) <= f32(1) / wc[0] <= f32(127.5)


def test_row_without_an_ok_element():
    weights8, wc = compress([[np.nan, np.inf, 0]])
    assert weights8.tolist() == [[0, 255, 0]]
    assert wc[0] == 0 and not np.signbit(wc[0])


def test_row_whose_scale_underflows():
    weights8, wc = compress([[TINY, 3 * TINY]])
    assert weights8.tolist() == [[255, 255]]
    assert wc[0] == 0 and not np.signbit(wc[0])


def test_rows_are_independent():
    weights8, wc = compress([[1, 3, 4], [0, 0, 0], [255, 1, 0.4], [3, np.inf, -np.inf]])
    assert weights8.tolist() == [[64, 191, 255], [0, 0, 0], [255, 1, 1], [255, 255, 0]]
    assert wc.tolist() == [f32(4) / f32(255), 0, 1, f32(3) / f32(255)]


def test_expand():
    weights8 = np.array([[0, 1, 255], [7, 0, 128]], np.uint8)
    wc = np.array([0.25, 3.0], f32)
    out = host.CompressWeightsHost.expand(weights8, wc)
    assert out.dtype == f32
    assert out.tolist() == [[0, 0.25, 63.75], [21, 0, 384]]
    assert host.CompressWeightsHost().expand(weights8, wc).tolist() == out.tolist()


# ----------------------------------------------------------------------- the double loop
def double_loop(weights):
    """The issue's arithmetic, sample by sample, in np.float32 scalars."""
    channels, baselines = weights.shape
    weights8 = np.zeros((channels, baselines), np.uint8)
    weights_channel = np.zeros(channels, f32)
    with np.errstate(all="ignore"):
        for c in range(channels):
            m = f32(0)
            for b in range(baselines):
                w = weights[c, b]
                if w > 0 and w < np.inf and w > m:
                    m = w
            wc = f32(m / f32(255))
            weights_channel[c] = wc
            for b in range(baselines):
                w = weights[c, b]
                if not w > 0:
                    q = 0
                else:
                    t = f32(w / wc)
                    q = 255 if t >= 255 else max(1, int(np.rint(t)))
                weights8[c, b] = q
    return weights8, weights_channel


def loop_case(seed, channels, baselines):
    """2^U(-30, 30) with about 10 % zeros, some NaN, inf, negative and denormal values, the
    last row all zero."""
    rs = np.random.RandomState(seed)
    weights = np.exp2(rs.uniform(-30, 30, (channels, baselines))).astype(f32)
    kind = rs.random_sample(weights.shape)
    weights[kind < 0.10] = 0
    special = [np.nan, np.inf, -np.inf, -1.5, -0.0, TINY, 2.0**-130, 1e-39]
    for i, value in enumerate(special):
        weights[(kind >= 0.10 + 0.02 * i) & (kind < 0.12 + 0.02 * i)] = value
    weights[-1] = 0
    return weights


@pytest.mark.parametrize("channels, baselines", [(9, 13), (1, 1)])
def test_host_against_double_loop(channels, baselines):
    weights = loop_case(channels, channels, baselines)
    if channels > 1:
        assert np.isnan(weights).any() and np.isposinf(weights).any() and (weights < 0).any()
        assert ((weights > 0) & (weights < np.finfo(f32).tiny)).any()
        weights[1] = np.where(weights[1] > 0, TINY * f32(77), weights[1])  # an all-denormal row
        weights[2, 3] = 2.0**-120  # a denormal wc, unless a neighbour is larger
    want = double_loop(weights)
    got = host.CompressWeightsHost()(weights)
    same_bits(want[0], got[0])
    same_bits(want[1], got[1])
    assert not got[0][-1].any() and got[1][-1] == 0
    assert got[0].flags.c_contiguous


# --------------------------------------------------------------------------- properties
def test_properties_over_random_rows():
    """300 rows whose maximum is at least 2^-100 (a normal wc): the maximum maps to 255, the
    byte is 0 exactly where the weight is not positive, and what the consumer computes from
    the byte is within wc / 2 (1 + 2^-20) of the weight, within wc where the byte was held up
    to 1."""
    rs = np.random.RandomState(17)
    baselines = 97
    weights = np.exp2(rs.uniform(-30, 30, (300, baselines))).astype(f32)
    # rows of every level from 2^-100 up, and rows with a small dynamic range
    weights *= np.exp2(rs.randint(-70, 60, (300, 1))).astype(f32)
    narrow = rs.random_sample(300) < 0.3
    weights[narrow] = (rs.uniform(1, 300, (np.count_nonzero(narrow), baselines))).astype(f32)
    weights[rs.random_sample(weights.shape) < 0.10] = 0
    weights[rs.random_sample(weights.shape) < 0.02] = -1
    weights[rs.random_sample(weights.shape) < 0.02] = np.nan
    weights[:, 0] = np.maximum(np.nan_to_num(weights[:, 0]), f32(2.0**-100))
    assert np.isfinite(weights[~np.isnan(weights)]).all()
    weights8, wc = host.CompressWeightsHost()(weights)
    positive = weights > 0
    m = np.where(positive, weights, 0).max(axis=1)
    assert (m >= 2.0**-100).all() and (wc >= np.finfo(f32).tiny).all()
    at_max = positive & (weights == m[:, np.newaxis])
    assert at_max.any(axis=1).all() and (weights8[at_max] == 255).all()
    np.testing.assert_array_equal(weights8 == 0, ~positive)
    back = host.CompressWeightsHost.expand(weights8, wc).astype(np.float64)
    error = np.abs(back - weights.astype(np.float64))
    scale = np.broadcast_to(wc.astype(np.float64)[:, np.newaxis], weights.shape)
    many = positive & (weights8 > 1)
    one = positive & (weights8 == 1)
    assert np.count_nonzero(many) > 3000 and np.count_nonzero(one) > 3000
    assert (error[many] <= scale[many] / 2 * (1 + 2.0**-20)).all()
    assert (error[one] <= scale[one]).all()
    assert (back[~positive] == 0).all()


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    compress = host.CompressWeightsHost()
    weights = np.ones((4, 6), f32)
    compress(weights)
    for bad in (weights.astype(np.float64), weights.astype(np.int32), weights[0],
                weights[np.newaxis], np.zeros((0, 6), f32), np.zeros((4, 0), f32)):  # fmt: skip
        with pytest.raises(ValueError, match="weights"):
            compress(bad)
    weights8, wc = compress(weights)
    for name, bad in [("weights8", weights8.astype(np.int8)), ("weights8", weights8[0]),
                      ("weights_channel", wc.astype(np.float64)), ("weights_channel", wc[:3]),
                      ("weights_channel", wc[:, np.newaxis])]:  # fmt: skip
        args = {"weights8": weights8, "weights_channel": wc}
        args[name] = bad
        with pytest.raises(ValueError, match=name):
            compress.expand(**args)


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.CompressWeightsTemplate(context, tuning={"wgs": 256})
    assert ingest.CompressWeightsTemplate(context, tuning={}).tuning == {}
    assert ingest.CompressWeightsTemplate.autotune(context) == {}
    assert ingest.CompressWeightsTemplate.host_class is host.CompressWeightsHost
    assert ingest.CompressWeightsTemplate.KERNEL == "ksp_compress_weights"
    template = ingest.CompressWeightsTemplate(context)
    assert template.kernel.name == "ksp_compress_weights"
    for args in [(0, 4), (4, 0), (-4, 4), (4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 4, 5), ingest.CompressWeights)
    assert isinstance(template.instantiate(queue, 1, 1), ingest.CompressWeights)


def test_host_from_device(context, queue):
    adapter = ingest.CompressWeightsHostFromDevice(ingest.CompressWeightsTemplate(context), queue)
    for bad in (np.ones(5, f32), np.ones((2, 3, 4), f32)):
        with pytest.raises(ValueError):
            adapter(bad)
    with pytest.raises(ValueError):
        adapter(np.ones((0, 5), f32))
    weights8, wc = adapter(np.ones((4, 5), f32))
    assert (weights8.shape, weights8.dtype) == ((4, 5), np.uint8)
    assert (wc.shape, wc.dtype) == ((4,), f32)
    assert [name for name, _ in queue.launches] == ["ksp_compress_weights"]
    assert [int(a) for a in queue.launches[0][1][3:5]] == [4, 5]


# ------------------------------------------------------------------------------- wiring
def test_wiring(context, queue):
    template = ingest.CompressWeightsTemplate(context)
    fn = template.instantiate(queue, 300, 200)
    shapes = {"weights": (300, 200), "weights8": (300, 200), "weights_channel": (300,)}
    dtypes = {"weights": np.float32, "weights8": np.uint8, "weights_channel": np.float32}
    assert set(fn.slots) == set(shapes)
    for name, shape in shapes.items():
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes[name]
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len(dims) == 5 and len({id(d) for d in dims}) == 5
    accel.Dimension(200, min_padded_size=500).link(fn.slots["weights8"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_compress_weights"]
    args = queue.launches[0][1]
    assert len(args) == 7
    assert args[0] is fn.buffer("weights").buffer
    assert args[1] is fn.buffer("weights8").buffer
    assert args[2] is fn.buffer("weights_channel").buffer
    assert all(isinstance(a, np.int32) for a in args[3:])
    assert [int(a) for a in args[3:5]] == [300, 200]
    assert fn.buffer("weights").padded_shape == (300, 224)  # whole 128-byte rows
    assert fn.buffer("weights8").padded_shape == (300, 512)
    assert [int(a) for a in args[5:]] == [224, 512]
    assert fn.parameters() == {"channels": 300, "baselines": 200}


def test_behind_finalise(context, queue):
    """finalise -> compress: `weights` is one buffer with one padded size."""
    channels, baselines, cf = 4096, 200, 8
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    compress = ingest.CompressWeightsTemplate(context).instantiate(
        queue, channels // cf, baselines)  # fmt: skip
    # more row padding than either asks for, asked of the other member of the compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("compress", compress)],
        compounds={"weights": ["finalise:weights", "compress:weights"]})  # fmt: skip
    assert "finalise:weights" not in seq.slots and "compress:weights" not in seq.slots
    assert {"weights", "compress:weights8", "compress:weights_channel", "finalise:vis",
            "finalise:flags"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_average_finalise", "ksp_compress_weights"]
    final_args, compress_args = (launch[1] for launch in queue.launches)
    assert finalise.buffer("weights") is compress.buffer("weights") is seq.buffer("weights")
    assert final_args[4] is compress_args[0] is seq.buffer("weights").buffer
    stride = seq.buffer("weights").padded_shape[1]
    assert stride == 320  # 300 rounded up to whole 128-byte rows
    assert int(final_args[14]) == int(compress_args[5]) == stride
    assert [int(a) for a in compress_args[3:5]] == [channels // cf, baselines]
    assert int(compress_args[6]) == seq.buffer("compress:weights8").padded_shape[1] == 256


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

    def call(weights=p, weights8=p, weights_channel=p, channels=4, baselines=8,
             weights_stride=8, weights8_stride=8):  # fmt: skip
        rc = lib.ksp_compress_weights(0, None, weights, weights8, weights_channel, channels,
                                      baselines, weights_stride, weights8_stride)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: weights is NULL" in call(weights=None)
    assert "invalid argument: weights8 is NULL" in call(weights8=None)
    assert "invalid argument: weights_channel is NULL" in call(weights_channel=None)
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    assert "invalid argument: weights_stride is smaller than baselines" in call(weights_stride=7)
    assert "invalid argument: weights8_stride is smaller than baselines" in call(weights8_stride=7)
    assert "weights8_stride is smaller" in call(baselines=70000, weights_stride=70000,
                                                weights8_stride=69999)  # fmt: skip
    # the order of the checks: everything wrong at once, then only every stride
    assert "invalid argument: weights is NULL" in call(
        weights=None, weights8=None, weights_channel=None, channels=0, baselines=0,
        weights_stride=-1, weights8_stride=-1)  # fmt: skip
    assert "invalid argument: weights_stride is smaller than baselines" in call(
        weights_stride=7, weights8_stride=7)  # fmt: skip
